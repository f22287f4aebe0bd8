"""PLDA log-likelihood-ratio scoring of the identify / verify decision: a window against an enrolled SPEAKER, not against single embeddings.

The rule (this build's statement; parity with Kaldi or any outside toolkit is unpinned).  Work in the space x = plda_transform(e) of a
plda.Plda (D = 64 or 128 columns): within-speaker covariance I, between-speaker covariance diag(Phi).  A speaker s owns several enrolled
embeddings; u_s is the mean of their transformed rows, added in ascending row order, and n_s > 0 an effective count given by the caller (the
number of enrolled embeddings - "by the book" - or 1).  Per column, with n = n_s:

    a = n Phi / (n Phi + 1)          the posterior mean of the speaker's centre is a u
    v = 1 + Phi / (n Phi + 1)        the predictive variance of a window of that speaker
    g = a / v      q = -(1 / v - 1 / (1 + Phi)) / 2      h = -a^2 / (2 v)      c(n) = -1/2 sum_d [ln v_d - ln(1 + Phi_d)]

    llr(x, s) = c(n_s) + sum_d x_d u_sd g_d(n_s) + sum_d x_d^2 q_d(n_s) + sum_d u_sd^2 h_d(n_s)
              = ln N(x | a u_s, v) - ln N(x | 0, 1 + Phi)

So the score matrix is one product of depth 2 D plus a constant per speaker: with Z = [x, x^2] [N, 2 D], the table G_s = [g(n_s) o u_s, q(n_s)]
[S, 2 D] and r_s = c(n_s) + sum_d u_sd^2 h_d(n_s):  llr = Z G^T + r.  Everything is float64.

  table    a speaker without a row, or whose n_s is not a finite number above 0, gets a G row of zeros and r = NaN: it never wins.  A label
           outside [0, S) belongs to no speaker.
  top-k    per window the k <= 4 largest llr, ties to the lowest speaker index; a NaN never wins; a slot without a candidate holds
           idx -1, score 0.
  decision a window votes for its top-1 speaker when llr >= threshold (a NaN does not).  The llr scale is UNCALIBRATED: 0 is the point of
           equal likelihood under the model, not a tuned operating point.  Backend.tune_verification (trials.py) finds one on a labelled
           development set: the thresholds at the equal error rate and at the minimum detection cost.

On the device: ops.Engine.plda_enroll and ops.Engine.plda_score_topk (csrc/plda_score.hip: the product on the f64 MFMA, x^2 formed in the
kernel, the speakers split across workgroups and merged in a fixed order).  This module holds the numpy float64 restatements for hosts that
post-process stored embeddings, the grouping of a profile batch's rows by speaker and the aggregation of per-window winners into result
rows (the voting loop is rules.py's, shared with the other two rules); it imports neither torch nor the library.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

from .rules import _mean, _tally

MAX_TOPK = 4                      # k of the top-k
MAX_SPEAKERS = 1 << 20            # speakers sdk_plda_enroll / sdk_plda_score_topk serve
MAX_ROWS = 1 << 22                # profile rows sdk_plda_enroll serves
MAX_WINDOWS = 65536               # windows per sdk_plda_score_topk call
DIMS = (64, 128)


def coefficients(Phi, n) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(g, q, h) [..., D] and c [...] of the rule for the spectrum Phi [D] and the effective count(s) n (a scalar or an array [...])."""
    Phi = np.asarray(Phi, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)[..., None]
    den = n * Phi + 1.0
    a = n * Phi / den
    v = 1.0 + Phi / den
    g = a / v
    q = -0.5 * (1.0 / v - 1.0 / (1.0 + Phi))
    h = -(a * a) / (2.0 * v)
    c = -0.5 * (np.log(v) - np.log(1.0 + Phi)).sum(axis=-1)
    return g, q, h, c


def speaker_table_host(Xp, group, n_eff, Phi) -> Tuple[np.ndarray, np.ndarray]:
    """The speaker table in numpy: Xp [P, D] transformed profile rows, group [P] (the speaker index of every row, in any order), n_eff [S],
    Phi [D] -> (G [S, 2 D], r [S])."""
    Xp = np.asarray(Xp, dtype=np.float64)
    Phi = np.asarray(Phi, dtype=np.float64)
    n_eff = np.asarray(n_eff, dtype=np.float64)
    group = np.asarray(group)
    if Xp.ndim != 2 or Phi.shape != (Xp.shape[1],) or group.shape != (Xp.shape[0],) or n_eff.ndim != 1 or n_eff.shape[0] < 1:
        raise ValueError(f"speaker_table_host: Xp {Xp.shape}, group {group.shape}, n_eff {n_eff.shape}, Phi {Phi.shape} do not belong together")
    S, D = int(n_eff.shape[0]), int(Xp.shape[1])
    inside = (group >= 0) & (group < S)
    sums = np.zeros((S, D))
    np.add.at(sums, group[inside].astype(np.int64), Xp[inside])            # unbuffered: every speaker's rows in ascending row order
    m = np.bincount(group[inside].astype(np.int64), minlength=S)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = (m > 0) & np.isfinite(n_eff) & (n_eff > 0)
        u = sums / np.maximum(m, 1)[:, None]
        g, q, h, c = coefficients(Phi, np.where(ok, n_eff, 1.0))
        G = np.where(ok[:, None], np.concatenate([g * u, q], axis=1), 0.0)
        r = np.where(ok, c + (u * u * h).sum(axis=1), np.nan)
    return np.ascontiguousarray(G), r


def llr_host(X, G, r) -> np.ndarray:
    """The score matrix [N, S] in numpy: X [N, D] transformed windows, (G, r) a speaker table."""
    X, G, r = np.asarray(X, dtype=np.float64), np.asarray(G, dtype=np.float64), np.asarray(r, dtype=np.float64)
    if X.ndim != 2 or G.ndim != 2 or G.shape[1] != 2 * X.shape[1] or r.shape != (G.shape[0],):
        raise ValueError(f"llr_host: X {X.shape}, G {G.shape}, r {r.shape} do not belong together")
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([X, X * X], axis=1) @ G.T + r[None, :]


def topk_host(L, k: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """The top-k of a score matrix L [N, S]: (idx [N, k] int32, score [N, k]); ties to the lower speaker, a NaN never taken, a slot without
    a candidate (the columns S .. k - 1 among them) holds (-1, 0)."""
    L = np.asarray(L, dtype=np.float64)
    k = int(k)
    if L.ndim != 2 or L.shape[1] < 1 or k < 1 or k > MAX_TOPK:
        raise ValueError(f"topk_host: L {L.shape}, k={k} (a [N, S >= 1] matrix and 1 <= k <= {MAX_TOPK})")
    N, S = L.shape
    bad = np.isnan(L)
    with np.errstate(invalid="ignore"):
        order = np.argsort(np.where(bad, np.inf, -L), axis=1, kind="stable")[:, :k]        # NaN last; ties to the lower speaker
    idx = np.full((N, k), -1, np.int32)
    sc = np.zeros((N, k))
    kw = order.shape[1]
    lost = np.take_along_axis(bad, order, 1)
    idx[:, :kw] = np.where(lost, -1, order)
    sc[:, :kw] = np.where(lost, 0.0, np.take_along_axis(L, order, 1))
    return idx, sc


def group_speakers(speaker_ids: Sequence[Any]):
    """The rows of a profile batch by speaker -> (group [P] int32: the speaker index of every row, speakers: the ids in order of first
    appearance, first [S] int64: every speaker's first row, counts [S] int64: their rows)."""
    index: Dict[Any, int] = {}
    group = np.zeros(len(speaker_ids), np.int32)
    first: List[int] = []
    for p, sid in enumerate(speaker_ids):
        s = index.setdefault(sid, len(index))
        if s == len(first):
            first.append(p)
        group[p] = s
    return group, list(index), np.asarray(first, np.int64), np.bincount(group, minlength=len(index)).astype(np.int64)


def confidence(llr: float) -> float:
    """1 / (1 + exp(-llr)) without overflow at either end."""
    llr = float(llr)
    if llr >= 0.0:
        return 1.0 / (1.0 + math.exp(-llr))
    e = math.exp(llr)
    return e / (1.0 + e)


def aggregate_matches_plda(best_idx, best_llr, spans, speakers, embedding_ids, counts, threshold: float) -> List[Dict[str, Any]]:
    """Per-window top-1 (speaker index, llr) -> one result row per matched speaker.  A window votes for its speaker when llr >= threshold
    (idx -1 and a NaN do not vote).  speakers [S]: the ids; embedding_ids [S]: every speaker's first embedding in batch order; counts [S]:
    their enrolled embeddings.  llr = the float64 mean of the speaker's voting windows' llr; similarity = confidence = 1 / (1 + exp(-llr));
    rows sorted by llr descending, then speaker id."""
    per = _tally((None if s < 0 or not l >= threshold else (s, l)
                  for s, l in zip(np.asarray(best_idx).tolist(), np.asarray(best_llr, dtype=np.float64).tolist())), spans)
    out = []
    for s, acc in per.items():
        llr = _mean(acc["votes"])
        conf = confidence(llr)
        out.append({"speaker_id": speakers[s], "llr": llr, "similarity": conf, "confidence": conf, "embedding_id": embedding_ids[s],
                    "n_embeddings": int(counts[s]), "segment": (acc["first"], acc["last"]), "n_segments": len(acc["votes"])})
    out.sort(key=lambda r: (-r["llr"], r["speaker_id"]))
    return out
