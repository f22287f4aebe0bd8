"""Verification trials: how well a decision rule of identify / verify separates same-speaker from different-speaker pairs - the equal error
rate, the minimum detection cost, the DET curve and the thresholds at both operating points - from a labelled set of embeddings.

The rule (this build's statement; parity with Kaldi's compute-eer / compute_min_dcf, pyannote.metrics or any outside toolkit is unpinned).

  trial    Test rows i < N against model rows j < M, with int32 labels la [N], lb [M] and int32 sessions sa [N], sb [M].  Trial (i, j) is
           EXCLUDED when la[i] < 0, or lb[j] < 0, or (sa[i] >= 0 and sa[i] == sb[j]) - a row is not scored against its own recording.
           Otherwise its class is target (1) when la[i] == lb[j], else nontarget (0).
  score    s(i, j) = r[j] + sum_k A[i, k] B[j, k] in float64; A [N, K], B [M, K], r [M], K a multiple of 16 in 16 .. 512, 1 <= N, M <= 2^20.
           cosine: A and B the unit embeddings widened to float64, r = 0 (K = 192 or 256).  PLDA: A = [x, x * x] of the transformed
           windows, (B, r) = (G, r) the speaker table of Engine.plda_enroll, K = 2 D (plda_score.py).
  integer  With finite lo < hi, scale = 2^24 / (hi - lo) formed once in float64.  t = (s - lo) * scale is ONE float64 subtraction, then ONE
  score    float64 multiplication (never an FMA).  A NaN is counted as nan; t < 0 is BELOW; t >= 2^24 (+inf included) is ABOVE; otherwise
           q = floor(t) in [0, 2^24).  q is non-decreasing in s, and every metric below is defined on q: the resolution is (hi - lo) / 2^24
           (1.2e-7 for cosine).
  a pass   has (shift, base): bin = (q >> shift) - base.  A trial that is neither excluded nor nan is counted exactly once: in
           hist[class][bin] when 0 <= bin < 4096, in under[class] when (q >> shift) < base or the score is below, in over[class] otherwise
           (above included).  Pass 1 is (12, 0): 4096 coarse bins of 4096 values of q.  A zoom into coarse bin b is (0, 4096 b).
  metrics  Accept when q >= t, for an integer t in [0, 2^24]: miss(t) = targets with q < t, plus the targets below; fa(t) = nontargets with
           q >= t, plus the nontargets above; T and Nn the class totals (ValueError when either is 0); nan trials are reported and left out
           of both.  Pmiss = miss / T, Pfa = fa / Nn.
           EER: t* = the least t with miss(t) Nn >= fa(t) T (exact integers) - its coarse bin from pass 1, t* itself from ONE zoom.  With
           t* = 0, eer = (Pmiss(0) + Pfa(0)) / 2; otherwise, between the points at t* - 1 and t*: d0 = Pfa(t* - 1) - Pmiss(t* - 1),
           d1 = Pmiss(t*) - Pfa(t*), eer = Pmiss(t* - 1) + d0 / (d0 + d1) (Pmiss(t*) - Pmiss(t* - 1)).  eer_threshold = lo + t* / scale.
           No t <= 2^24 with the condition: ValueError that names the over counts and asks for a wider range.
           minDCF (p_target, c_miss, c_fa; defaults 0.01, 1, 1): dcf(t) = (c_miss p Pmiss(t) + c_fa (1 - p) Pfa(t)) / min(c_miss p, c_fa (1 - p)).
           Candidates: the 4097 coarse thresholds, accept-all and reject-all.  Coarse bin b has the rigorous lower bound
           LB_b = (c_miss p Pmiss(4096 b) + c_fa (1 - p) Pfa(4096 (b + 1))) / min(..): inside the bin Pmiss is at least its value at the lower
           edge and Pfa at least its value at the upper edge.  The bins with LB_b below the best value so far are zoomed into in ascending
           LB_b, at most max_refine of them (default 8); a zoom replaces the bin's bound by its exact minimum over its 4096 thresholds.
           min_dcf = the best value found (an upper bound of the minimum), min_dcf_lower = the least remaining bound, min_dcf_exact = the
           two are equal, min_dcf_threshold = lo + t / scale of the best (-inf: accept all, +inf: reject all).
           DET: pmiss, pfa at the 4097 coarse thresholds, and those thresholds in score units.

On the device: ops.Engine.trial_hist (csrc/trials.hip: the product tile by tile on the f64 MFMA, every tile straight into a two-class integer
histogram in LDS; the score matrix is never written).  Everything after the product is integer arithmetic: the counts are bit-identical run
to run.  This module holds the numpy restatement of a pass, the metric functions on counts and the driver of pass 1 and the zooms; it imports
neither torch nor the library at module level.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np

BINS = 4096
Q_BITS = 24
Q_MAX = 1 << Q_BITS                # thresholds are the integers 0 .. Q_MAX
COARSE_SHIFT = 12
MAX_ROWS = 1 << 20
COSINE_RANGE = (-1.0 - 2.0 ** -16, 1.0 + 2.0 ** -16)
PLDA_RANGE = (-1024.0, 1024.0)


class PassCounts(NamedTuple):
    """The 8199 counters of one pass, on the host."""
    hist: np.ndarray               # [2, 4096] int64
    under: np.ndarray              # [2]
    over: np.ndarray               # [2]
    nan: np.ndarray                # [2]
    excluded: int

    def total(self) -> int:
        return int(self.hist.sum()) + int(self.under.sum()) + int(self.over.sum())


def scale_of(lo: float, hi: float) -> float:
    """2^24 / (hi - lo) in float64 for finite lo < hi (ValueError otherwise, and when the quotient is not a finite number above 0)."""
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"score range ({lo}, {hi}): finite lo < hi expected")
    with np.errstate(over="ignore"):
        scale = float(np.float64(Q_MAX) / (np.float64(hi) - np.float64(lo)))
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"score range ({lo}, {hi}): scale = 2^24 / (hi - lo) = {scale} is not a finite number above 0")
    return scale


def counts_from_scores(S, cls, lo: float, hi: float, shift: int = COARSE_SHIFT, base: int = 0) -> PassCounts:
    """One pass over a score array S (any shape, float64) with classes cls (same shape: 1 target, 0 nontarget, negative = excluded)."""
    S = np.asarray(S, dtype=np.float64).ravel()
    cls = np.asarray(cls).ravel()
    scale = scale_of(lo, hi)
    shift, base = int(shift), int(base)
    if not (0 <= shift <= Q_BITS and 0 <= base <= Q_MAX):
        raise ValueError(f"shift={shift} (0 .. 24), base={base} (0 .. 2^24)")
    keep = cls >= 0
    excluded = int((~keep).sum())
    S, cls = S[keep], cls[keep].astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (S - np.float64(lo)) * np.float64(scale)
    isnan = np.isnan(t)
    below = ~isnan & (t < 0.0)
    above = ~isnan & (t >= float(Q_MAX))
    inside = ~(isnan | below | above)
    qs = np.zeros(t.shape, np.int64)
    qs[inside] = np.floor(t[inside]).astype(np.int64) >> shift
    under = below | (inside & (qs < base))
    binned = inside & (qs >= base) & (qs - base < BINS)
    over = ~(isnan | under | binned)
    hist = np.zeros((2, BINS), np.int64)
    for c in (0, 1):
        hist[c] = np.bincount((qs - base)[binned & (cls == c)], minlength=BINS)
    two = lambda m: np.asarray([int((m & (cls == 0)).sum()), int((m & (cls == 1)).sum())], np.int64)        # noqa: E731
    return PassCounts(hist, two(under), two(over), two(isnan), excluded)


def trial_classes(la, sa, lb, sb) -> np.ndarray:
    """The class of every trial [N, M]: 1 target, 0 nontarget, -1 excluded."""
    la, sa, lb, sb = (np.asarray(a).astype(np.int64) for a in (la, sa, lb, sb))
    excl = (la[:, None] < 0) | (lb[None, :] < 0) | ((sa[:, None] >= 0) & (sa[:, None] == sb[None, :]))
    return np.where(excl, -1, (la[:, None] == lb[None, :]).astype(np.int64))


def trial_hist_host(A, B, r, la, sa, lb, sb, lo: float, hi: float, shift: int = COARSE_SHIFT, base: int = 0) -> PassCounts:
    """The numpy restatement of Engine.trial_hist: the float64 product A @ B.T + r, then one pass."""
    A, B, r = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64), np.asarray(r, dtype=np.float64)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or r.shape != (B.shape[0],):
        raise ValueError(f"trial_hist_host: A {A.shape}, B {B.shape}, r {r.shape} do not belong together")
    with np.errstate(invalid="ignore", over="ignore"):
        S = A @ B.T + r[None, :]
    return counts_from_scores(S, trial_classes(la, sa, lb, sb), lo, hi, shift, base)


# ---- metrics on counts ---------------------------------------------------------------------------------------------------------------------
def _ints(a):
    return [int(v) for v in np.asarray(a).tolist()]


def _cumulative(p: PassCounts):
    """miss and fa (Python integers) at the 4097 thresholds of a pass: threshold e is "the least q of bin e" (e = 4096: past the last bin)."""
    h0, h1 = _ints(p.hist[0]), _ints(p.hist[1])
    miss = [int(p.under[1])]
    for v in h1:
        miss.append(miss[-1] + v)
    fa = [int(p.over[0])]
    for v in reversed(h0):
        fa.append(fa[-1] + v)
    fa.reverse()
    return miss, fa


def totals(p: PassCounts) -> Tuple[int, int]:
    """(T, Nn): the targets and nontargets of a pass (nan and excluded trials are in neither); ValueError when either is 0."""
    T = int(p.hist[1].sum()) + int(p.under[1]) + int(p.over[1])
    Nn = int(p.hist[0].sum()) + int(p.under[0]) + int(p.over[0])
    if T == 0 or Nn == 0:
        raise ValueError(f"verification trials need both classes: {T} target and {Nn} nontarget trials "
                         f"({int(p.nan.sum())} NaN, {int(p.excluded)} excluded)")
    return T, Nn


def _check_zoom(coarse: PassCounts, fine: PassCounts, b: int) -> None:
    if fine.total() != coarse.total() or int(fine.hist[0].sum()) != int(coarse.hist[0][b]) or int(fine.hist[1].sum()) != int(coarse.hist[1][b]):
        raise RuntimeError(f"the zoom into coarse bin {b} does not account for the trials of pass 1 (are both passes of the same data and range?)")


def eer_from_counts(coarse: PassCounts, zoom: Callable[[int], PassCounts], lo: float, hi: float) -> Dict[str, Any]:
    """The equal error rate from pass 1 (coarse) and ONE zoom: zoom(b) returns the pass (0, 4096 b) of the same data and range.
    -> {"eer", "eer_threshold", "t_star", "pmiss", "pfa": the two rates at t*}."""
    scale = scale_of(lo, hi)
    T, Nn = totals(coarse)
    miss, fa = _cumulative(coarse)
    bstar = next((b for b in range(BINS + 1) if miss[b] * Nn >= fa[b] * T), None)
    if bstar is None:
        raise ValueError(f"the miss and false-alarm curves do not cross inside the score range ({lo}, {hi}): {int(coarse.over[1])} target and "
                         f"{int(coarse.over[0])} nontarget trials lie above it (over); pass a wider score_range")
    if bstar == 0:
        pm, pf = miss[0] / T, fa[0] / Nn
        return {"eer": (pm + pf) / 2, "eer_threshold": lo + 0 / scale, "t_star": 0, "pmiss": pm, "pfa": pf}
    b = bstar - 1
    fine = zoom(b)
    _check_zoom(coarse, fine, b)
    fmiss, ffa = _cumulative(fine)
    j = next(j for j in range(BINS + 1) if fmiss[j] * Nn >= ffa[j] * T)          # true at 4096 (= coarse threshold bstar), false at 0
    pm0, pf0, pm1, pf1 = fmiss[j - 1] / T, ffa[j - 1] / Nn, fmiss[j] / T, ffa[j] / Nn
    d0, d1 = pf0 - pm0, pm1 - pf1
    t_star = BINS * b + j
    return {"eer": pm0 + (d0 / (d0 + d1) if d0 + d1 > 0 else 0.0) * (pm1 - pm0), "eer_threshold": lo + t_star / scale, "t_star": t_star, "pmiss": pm1, "pfa": pf1}


def _dcf(miss: int, fa: int, T: int, Nn: int, p: float, cm: float, cf: float) -> float:
    return (cm * p * (miss / T) + cf * (1 - p) * (fa / Nn)) / min(cm * p, cf * (1 - p))


def min_dcf_from_counts(coarse: PassCounts, zoom: Callable[[int], PassCounts], lo: float, hi: float, p_target: float = 0.01, c_miss: float = 1.0,
                        c_fa: float = 1.0, max_refine: int = 8) -> Dict[str, Any]:
    """The minimum normalised detection cost from pass 1 and at most max_refine zooms
    -> {"min_dcf", "min_dcf_lower", "min_dcf_exact", "min_dcf_threshold", "t_best", "n_zooms"}."""
    p, cm, cf = float(p_target), float(c_miss), float(c_fa)
    if not (0.0 < p < 1.0 and cm > 0.0 and cf > 0.0 and math.isfinite(cm) and math.isfinite(cf)):
        raise ValueError(f"min_dcf: p_target={p} (inside (0, 1)), c_miss={cm}, c_fa={cf} (finite, above 0)")
    scale = scale_of(lo, hi)
    T, Nn = totals(coarse)
    miss, fa = _cumulative(coarse)
    best, t_best = math.inf, None
    for b in range(BINS + 1):
        v = _dcf(miss[b], fa[b], T, Nn, p, cm, cf)
        if v < best:
            best, t_best = v, BINS * b
    for v, t in ((_dcf(0, Nn, T, Nn, p, cm, cf), -math.inf), (_dcf(T, 0, T, Nn, p, cm, cf), math.inf)):      # accept all, reject all
        if v < best:
            best, t_best = v, t
    bound = {b: _dcf(miss[b], fa[b + 1], T, Nn, p, cm, cf) for b in range(BINS) if coarse.hist[0][b] or coarse.hist[1][b]}
    n_zooms = 0
    while n_zooms < int(max_refine):
        open_bins = [(lb, b) for b, lb in bound.items() if lb < best]
        if not open_bins:
            break
        _, b = min(open_bins)
        fine = zoom(b)
        _check_zoom(coarse, fine, b)
        n_zooms += 1
        fmiss, ffa = _cumulative(fine)
        for j in range(BINS):
            v = _dcf(fmiss[j], ffa[j], T, Nn, p, cm, cf)
            if v < best:
                best, t_best = v, BINS * b + j
        del bound[b]                                     # its exact minimum is in `best` now
    lower = min([best] + [lb for lb in bound.values()])
    thr = t_best if isinstance(t_best, float) else lo + t_best / scale
    return {"min_dcf": best, "min_dcf_lower": lower, "min_dcf_exact": lower == best, "min_dcf_threshold": thr, "t_best": t_best, "n_zooms": n_zooms}


def det_from_counts(coarse: PassCounts, lo: float, hi: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The DET curve at the 4097 coarse thresholds -> (pmiss, pfa, thresholds in score units)."""
    scale = scale_of(lo, hi)
    T, Nn = totals(coarse)
    miss, fa = _cumulative(coarse)
    return (np.asarray([m / T for m in miss]), np.asarray([f / Nn for f in fa]), np.asarray([lo + (BINS * b) / scale for b in range(BINS + 1)]))


@dataclass
class VerificationResult:
    kind: str
    score_range: Tuple[float, float]
    counts: PassCounts                                   # pass 1
    n_target: int
    n_nontarget: int
    n_nan: int
    n_excluded: int
    eer: float
    eer_threshold: float
    min_dcf: float
    min_dcf_lower: float
    min_dcf_exact: bool
    min_dcf_threshold: float
    p_target: float
    c_miss: float
    c_fa: float
    det_pmiss: np.ndarray = field(repr=False)
    det_pfa: np.ndarray = field(repr=False)
    det_thresholds: np.ndarray = field(repr=False)
    n_zooms: int = 0
    t_star: int = 0
    t_best: Any = None
    test_rows: int = 0                                   # N and M of the trial matrix (set by the device driver)
    model_rows: int = 0


def result_from_passes(coarse: PassCounts, zoom: Callable[[int], PassCounts], kind: str, lo: float, hi: float, p_target: float = 0.01,
                       c_miss: float = 1.0, c_fa: float = 1.0, max_refine: int = 8) -> VerificationResult:
    """Every metric of the rule from pass 1 and a zoom callback (a zoom asked for twice is computed once)."""
    done: Dict[int, PassCounts] = {}

    def cached(b: int) -> PassCounts:
        if b not in done:
            done[b] = zoom(b)
        return done[b]

    T, Nn = totals(coarse)
    e = eer_from_counts(coarse, cached, lo, hi)
    d = min_dcf_from_counts(coarse, cached, lo, hi, p_target, c_miss, c_fa, max_refine)
    pm, pf, th = det_from_counts(coarse, lo, hi)
    return VerificationResult(kind=kind, score_range=(float(lo), float(hi)), counts=coarse, n_target=T, n_nontarget=Nn, n_nan=int(coarse.nan.sum()),
                              n_excluded=int(coarse.excluded), eer=e["eer"], eer_threshold=e["eer_threshold"], min_dcf=d["min_dcf"],
                              min_dcf_lower=d["min_dcf_lower"], min_dcf_exact=d["min_dcf_exact"], min_dcf_threshold=d["min_dcf_threshold"],
                              p_target=float(p_target), c_miss=float(c_miss), c_fa=float(c_fa), det_pmiss=pm, det_pfa=pf, det_thresholds=th,
                              n_zooms=len(done), t_star=e["t_star"], t_best=d["t_best"])


# ---- the device driver -----------------------------------------------------------------------------------------------------------------------
def counts_to_host(dev) -> PassCounts:
    """Engine.trial_hist's device tensors -> PassCounts (this is where the host waits for the pass)."""
    hist, under, over, nan, excluded = (t.cpu().numpy() for t in dev)
    return PassCounts(hist.astype(np.int64), under.astype(np.int64), over.astype(np.int64), nan.astype(np.int64), int(excluded[0]))


def evaluate_scores(engine, A, B, r, la, sa, lb, sb, kind: str, score_range: Optional[Tuple[float, float]] = None, p_target: float = 0.01,
                    c_miss: float = 1.0, c_fa: float = 1.0, max_refine: int = 8, max_blocks: int = 0) -> VerificationResult:
    """Pass 1 and the zooms on the device for trials already in matrix form (device tensors as Engine.trial_hist takes them)."""
    if kind not in ("cosine", "plda"):
        raise ValueError(f"evaluate: kind={kind!r} ('cosine' or 'plda')")
    lo, hi = score_range if score_range is not None else (COSINE_RANGE if kind == "cosine" else PLDA_RANGE)
    scale_of(lo, hi)

    def run(shift: int, base: int) -> PassCounts:
        return counts_to_host(engine.trial_hist(A, B, r, la, sa, lb, sb, lo, hi, shift=shift, base=base, max_blocks=max_blocks))

    coarse = run(COARSE_SHIFT, 0)
    res = result_from_passes(coarse, lambda b: run(0, BINS * b), kind, lo, hi, p_target, c_miss, c_fa, max_refine)
    res.test_rows, res.model_rows = int(A.shape[0]), int(B.shape[0])
    return res


def _i32(engine_device, a, n: int, name: str):
    import torch
    a = np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"evaluate: {name} must be {n} integers, got {a.shape} {a.dtype}")
    if len(a) and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f"evaluate: {name} must fit int32")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(engine_device)


def plda_model_rows(engine, E_model, model_labels, model_sessions, plda, count_by_book: bool = True):
    """The model side of PLDA trials: the rows with a label >= 0 grouped by label (ascending), pooled by Engine.plda_enroll
    -> (G [S, 2 D], r [S] device tensors, labels [S], sessions [S] numpy int32).  A speaker's session is its rows' common session, else -1.
    count_by_book: a speaker's effective count is the number of its rows (else 1)."""
    import torch
    labels = np.asarray(model_labels).astype(np.int64)
    sessions = np.asarray(model_sessions).astype(np.int64)
    keep = np.flatnonzero(labels >= 0)
    if not len(keep):
        raise ValueError("evaluate: no model row has a label >= 0")
    speakers, group = np.unique(labels[keep], return_inverse=True)
    counts = np.bincount(group, minlength=len(speakers))
    sess = np.full(len(speakers), -1, np.int64)
    for s in range(len(speakers)):
        own = np.unique(sessions[keep][group == s])
        if len(own) == 1:
            sess[s] = own[0]
    dev = E_model.device
    rows = torch.from_numpy(keep.astype(np.int32)).to(dev)
    Xp = torch.cat([engine.plda_transform(E_model, rows[a:a + 65536], plda, check_rows=False) for a in range(0, len(keep), 65536)], dim=0)
    n_eff = counts.astype(np.float64) if count_by_book else np.ones(len(speakers), np.float64)
    G, r, _ = engine.plda_enroll(Xp, torch.from_numpy(group.astype(np.int32)).to(dev), torch.from_numpy(n_eff).to(dev),
                                 plda.device_arrays(dev)["Phi"])                  # the groups lie in [0, S): status is not read
    return G, r, speakers.astype(np.int32), sess.astype(np.int32)


def plda_test_rows(engine, E_test, plda):
    """fp32 unit rows [N, d] (device) -> A = [x, x * x] [N, 2 D] float64 in the model's space."""
    import torch
    n = int(E_test.shape[0])
    parts = [engine.plda_transform(E_test, torch.arange(a, min(n, a + 65536), dtype=torch.int32, device=E_test.device), plda, check_rows=False)
             for a in range(0, n, 65536)]
    X = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
    return torch.cat([X, X * X], dim=1).contiguous()


def evaluate(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, kind: str = "cosine", plda=None, count_by_book: bool = True,
             score_range: Optional[Tuple[float, float]] = None, p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0,
             max_refine: int = 8, max_blocks: int = 0) -> VerificationResult:
    """Every test row against every model row under one decision rule -> VerificationResult.  E_test [N, d], E_model [P, d]: fp32 unit rows
    on the device; labels, sessions [N] and model_labels, model_sessions [P]: integers (a negative label: the row takes part in no trial;
    session -1: no session).  kind="cosine": the model rows are scored one by one (d a multiple of 16).  kind="plda": `plda` is a plda.Plda
    of this embedding space; the model rows are grouped by label into speakers and pooled (Engine.plda_enroll, count_by_book as
    SDK_SCORE_PLDA_COUNT), the trials are test rows against SPEAKERS.  score_range defaults to (-1 - 2^-16, 1 + 2^-16) for cosine and
    (-1024, 1024) for PLDA."""
    import torch
    if not (isinstance(E_test, torch.Tensor) and isinstance(E_model, torch.Tensor) and E_test.is_cuda and E_model.is_cuda and E_test.dim() == 2
            and E_model.dim() == 2 and E_test.shape[1] == E_model.shape[1] and E_test.dtype == torch.float32 and E_model.dtype == torch.float32):
        raise ValueError("evaluate: E_test [N, d] and E_model [P, d] must be fp32 device tensors of one width")
    N, P, dev = int(E_test.shape[0]), int(E_model.shape[0]), E_test.device
    la, sa = _i32(dev, labels, N, "labels"), _i32(dev, sessions, N, "sessions")
    if kind == "cosine":
        A, B = E_test.contiguous().double(), E_model.contiguous().double()
        r = torch.zeros((P,), dtype=torch.float64, device=dev)
        lb, sb = _i32(dev, model_labels, P, "model_labels"), _i32(dev, model_sessions, P, "model_sessions")
    elif kind == "plda":
        if plda is None:
            raise ValueError("evaluate: kind='plda' needs a plda.Plda model (plda=)")
        E_model = E_model.contiguous()
        G, r, spk, sess = plda_model_rows(engine, E_model, np.asarray(_i32("cpu", model_labels, P, "model_labels")),
                                          np.asarray(_i32("cpu", model_sessions, P, "model_sessions")), plda, count_by_book)
        A, B = plda_test_rows(engine, E_test.contiguous(), plda), G
        lb, sb = torch.from_numpy(spk).to(dev), torch.from_numpy(sess).to(dev)
    else:
        raise ValueError(f"evaluate: kind={kind!r} ('cosine' or 'plda')")
    return evaluate_scores(engine, A, B, r, la, sa, lb, sb, kind, score_range, p_target, c_miss, c_fa, max_refine, max_blocks)
