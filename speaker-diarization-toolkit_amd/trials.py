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

Calibration: an affine map llr = a s + b from the score s of a decision rule to a log-likelihood ratio, fitted by prior-weighted
logistic regression on labelled trials, and the cost of the log-likelihood ratio (Cllr) before and after (this build's statement; parity
with BOSARIS, Kaldi or any outside toolkit is unpinned, as for the metrics above).

  trials     Trials, classes, exclusions and the score s(i, j) are exactly those of the rule above.  A trial whose score is not finite
             (NaN, +inf or -inf) is counted in nonfinite[class] and left out of every sum; excluded trials are counted in `excluded`.
  a pass     takes (a, c).  With y = +1 for a target and -1 for a nontarget:
               z = a * s + c      ONE float64 multiplication, then ONE float64 addition (never an FMA)
               m = y z,  e = exp(-|m|)
               loss = max(-m, 0) + log1p(e)                           the stable form of softplus(-m)
               p = e / (1 + e),  q = 1 / (1 + e),  w = p when m >= 0, else q      w = sigmoid(-m)
               v = p * q                                              w (1 - w); 1 - w is the OTHER quotient, never a subtraction (for m far
                                                                      below 0 the subtraction would cancel: w rounds to 1)
             Per class the pass returns the count n of the trials summed and seven float64 sums over them:
               L = sum loss, W0 = sum w, W1 = sum w s, H0 = sum v, H1 = sum v s, H2 = sum (v s) s, S1 = sum s
             and nonfinite[2], excluded.
  objective  The effective prior P = p c_miss / (p c_miss + (1 - p) c_fa) (defaults as minDCF: 0.01, 1, 1), theta = ln(P / (1 - P)).
               J(a, b) = P L_1 / n_1 + (1 - P) L_0 / n_0    at c = b + theta
             d loss / dm = -w and d2 loss / dm2 = v, with dm/da = y s and dm/db = y, so with u_1 = P / n_1 and u_0 = (1 - P) / n_0:
               dJ/da = u_0 W1_0 - u_1 W1_1        dJ/db = u_0 W0_0 - u_1 W0_1
               Haa = u_0 H2_0 + u_1 H2_1          Hab = u_0 H1_0 + u_1 H1_1          Hbb = u_0 H0_0 + u_1 H0_1
               Cllr(a, b) = (L_1 / n_1 + L_0 / n_0) / (2 ln 2)    at c = b
  fit        Start: the minimiser of J on pass 1's coarse counts - the 4096 bin centres in score units with the counts as weights, the
             trials in under / over at lo / hi (host only).  Then damped Newton on the device sums: the step -H^-1 grad (the gradient
             itself when H is not positive definite) is halved until the point it leads to has a J that is not above the current one
             (8 x 2^-53 of it are allowed for the rounding of J at the minimum); every point tried costs one pass.  Stop when both gradient components are at most
             grad_tol (1e-10) times J in magnitude, or after max_passes (24) passes of the iteration.  Separable classes have no finite
             minimiser: the result then says converged = False.  ValueError when either class is empty.
  reported   cllr_raw: one pass at (1, 0).  cllr: one pass at (a, b).  min_cllr_coarse: the minimum Cllr of the COARSELY QUANTISED score -
             pool-adjacent-violators on pass 1's bins (under, the 4096 bins, over: 4098 cells in score order), each pooled block's
             log-likelihood ratio ln(T_g Nn / (N_g T)); a bound that any monotone map of the 4096-bin score can reach, not the minimum over
             the unquantised score.  bayes_threshold = (-theta - b) / a in score units.  act_dcf: the normalised DCF of the metrics above at
             the integer threshold q(bayes_threshold) (0 when it lies below lo, 2^24 at or above hi), exact from pass 1 and one zoom;
             min_dcf beside it.  n_passes counts every pass: the two reported ones and the iteration's.

On the device: ops_score.trial_calib (csrc/trials.hip, tr_calib_kernel: trial_hist's tiling and product, the sums formed in the product's
epilogue in a fixed order without a float atomic - bit-identical run to run, a function of the inputs and the grid alone).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import TYPE_CHECKING, Any, Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np

if TYPE_CHECKING:
    from .backend import Backend

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


def trial_tensors(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, kind: str = "cosine", plda=None, count_by_book: bool = True):
    """The trials of evaluate / calibrate in matrix form -> (A, B, r, la, sa, lb, sb) device tensors (evaluate states the arguments)."""
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
    return A, B, r, la, sa, lb, sb


def evaluate(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, kind: str = "cosine", plda=None, count_by_book: bool = True,
             score_range: Optional[Tuple[float, float]] = None, p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0,
             max_refine: int = 8, max_blocks: int = 0) -> VerificationResult:
    """Every test row against every model row under one decision rule -> VerificationResult.  E_test [N, d], E_model [P, d]: fp32 unit rows
    on the device; labels, sessions [N] and model_labels, model_sessions [P]: integers (a negative label: the row takes part in no trial;
    session -1: no session).  kind="cosine": the model rows are scored one by one (d a multiple of 16).  kind="plda": `plda` is a plda.Plda
    of this embedding space; the model rows are grouped by label into speakers and pooled (Engine.plda_enroll, count_by_book as
    SDK_SCORE_PLDA_COUNT), the trials are test rows against SPEAKERS.  score_range defaults to (-1 - 2^-16, 1 + 2^-16) for cosine and
    (-1024, 1024) for PLDA."""
    tensors = trial_tensors(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, kind, plda, count_by_book)
    return evaluate_scores(engine, *tensors, kind, score_range, p_target, c_miss, c_fa, max_refine, max_blocks)


# ---- calibration: what a score means ---------------------------------------------------------------------------------------------------------


class CalibSums(NamedTuple):
    """One calibration pass on the host; row 0 nontarget, row 1 target; the sums in the order L, W0, W1, H0, H1, H2, S1."""
    n: np.ndarray                  # [2] int64
    sums: np.ndarray               # [2, 7] float64
    nonfinite: np.ndarray          # [2] int64
    excluded: int


def effective_prior(p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0) -> float:
    p, cm, cf = float(p_target), float(c_miss), float(c_fa)
    if not (0.0 < p < 1.0 and cm > 0.0 and cf > 0.0 and math.isfinite(cm) and math.isfinite(cf)):
        raise ValueError(f"calibrate: p_target={p} (inside (0, 1)), c_miss={cm}, c_fa={cf} (finite, above 0)")
    return p * cm / (p * cm + (1.0 - p) * cf)


def _terms(s: np.ndarray, y: np.ndarray, a: float, c: float) -> np.ndarray:
    """The seven terms [7, n] of finite float64 scores s with y = +1 / -1, operation for operation as the kernel forms them."""
    with np.errstate(over="ignore", invalid="ignore"):
        z = np.float64(a) * s + np.float64(c)              # numpy rounds the product, then the sum
        m = y * z
        e = np.exp(-np.abs(m))
        d = 1.0 + e
        p, q = e / d, 1.0 / d
        w = np.where(m >= 0.0, p, q)
        v = p * q
        vs = v * s
        return np.stack([np.maximum(-m, 0.0) + np.log1p(e), w, w * s, v, vs, vs * s, s])


def calib_sums_host(S, cls, a: float, c: float, weights=None) -> CalibSums:
    """The numpy restatement of a calibration pass over a score array S (any shape) with classes cls (1 target, 0 nontarget, negative =
    excluded).  weights (same shape, non-negative integers; default 1): a score stands for that many trials (fit_from_counts)."""
    S = np.asarray(S, dtype=np.float64).ravel()
    cls = np.asarray(cls).ravel()
    wt = np.ones(S.shape, np.int64) if weights is None else np.asarray(weights).ravel().astype(np.int64)
    keep = cls >= 0
    excluded = int(wt[~keep].sum())
    S, cls, wt = S[keep], cls[keep].astype(np.int64), wt[keep]
    fin = np.isfinite(S)
    n, sums, nonfinite = np.zeros(2, np.int64), np.zeros((2, 7), np.float64), np.zeros(2, np.int64)
    for k in (0, 1):
        sel = cls == k
        nonfinite[k] = int(wt[sel & ~fin].sum())
        s, g = S[sel & fin], wt[sel & fin]
        n[k] = int(g.sum())
        if len(s):
            t = _terms(s, np.full(s.shape, 1.0 if k else -1.0), a, c)
            sums[k] = (t * g[None, :]).sum(axis=1) if weights is not None else t.sum(axis=1)
    return CalibSums(n, sums, nonfinite, excluded)


def objective(cs: CalibSums, prior: float):
    """J, its gradient [2] and Hessian [2, 2] in (a, b) from the sums of a pass at c = b + theta (the docstring's formulas)."""
    n0, n1 = int(cs.n[0]), int(cs.n[1])
    if n0 == 0 or n1 == 0:
        raise ValueError(f"calibration needs both classes: {n1} target and {n0} nontarget trials with a finite score "
                         f"({int(np.sum(cs.nonfinite))} not finite, {int(cs.excluded)} excluded)")
    u0, u1 = (1.0 - prior) / n0, prior / n1
    x0, x1 = cs.sums[0], cs.sums[1]
    J = u1 * x1[0] + u0 * x0[0]
    g = np.asarray([u0 * x0[2] - u1 * x1[2], u0 * x0[1] - u1 * x1[1]])
    H = np.asarray([[u0 * x0[5] + u1 * x1[5], u0 * x0[4] + u1 * x1[4]], [u0 * x0[4] + u1 * x1[4], u0 * x0[3] + u1 * x1[3]]])
    return float(J), g, H


def cllr_of(cs: CalibSums) -> float:
    """Cllr from the sums of a pass at c = b."""
    n0, n1 = int(cs.n[0]), int(cs.n[1])
    if n0 == 0 or n1 == 0:
        raise ValueError(f"Cllr needs both classes: {n1} target and {n0} nontarget trials with a finite score")
    return float((cs.sums[1][0] / n1 + cs.sums[0][0] / n0) / (2.0 * math.log(2.0)))


class FitResult(NamedTuple):
    a: float
    b: float
    J: float
    grad: Tuple[float, float]
    n_passes: int
    converged: bool


def newton_fit(sums: Callable[[float, float], CalibSums], a0: float, b0: float, prior: float, grad_tol: float = 1e-10,
               max_passes: int = 24) -> FitResult:
    """The damped Newton iteration of the rule from (a0, b0); sums(a, c) is one pass."""
    theta = math.log(prior / (1.0 - prior))
    a, b = float(a0), float(b0)
    J, g, H = objective(sums(a, b + theta), prior)
    passes = 1
    met = lambda J, g: math.isfinite(J) and J > 0.0 and bool(np.all(np.abs(g) <= grad_tol * J))        # noqa: E731
    while not met(J, g) and passes < max_passes:
        det = H[0, 0] * H[1, 1] - H[0, 1] * H[1, 0]
        if math.isfinite(det) and det > 0.0 and H[0, 0] > 0.0:
            step = -np.asarray([H[1, 1] * g[0] - H[0, 1] * g[1], H[0, 0] * g[1] - H[1, 0] * g[0]]) / det
        else:
            step = -g
        if not np.all(np.isfinite(step)):
            break
        t, moved = 1.0, False
        while passes < max_passes:
            na, nb = a + t * step[0], b + t * step[1]
            nJ, ng, nH = objective(sums(na, nb + theta), prior)
            passes += 1
            if nJ <= J * (1.0 + 8.0 * 2.0 ** -53):
                a, b, J, g, H, moved = na, nb, nJ, ng, nH, True
                break
            t *= 0.5
        if not moved:
            break
    return FitResult(a, b, J, (float(g[0]), float(g[1])), passes, met(J, g) and math.isfinite(a) and math.isfinite(b))


def _coarse_points(coarse: PassCounts, lo: float, hi: float):
    """Pass 1 as weighted scores: under at lo, the 4096 bin centres, over at hi -> (x [4098], targets [4098], nontargets [4098])."""
    scale = scale_of(lo, hi)
    centres = lo + (BINS * np.arange(BINS) + BINS // 2) / scale
    x = np.concatenate([[float(lo)], centres, [float(hi)]])
    cnt = lambda k: np.concatenate([[int(coarse.under[k])], coarse.hist[k].astype(np.int64), [int(coarse.over[k])]])        # noqa: E731
    return x, cnt(1), cnt(0)


def fit_from_counts(coarse: PassCounts, lo: float, hi: float, prior: float, grad_tol: float = 1e-10, max_passes: int = 64) -> FitResult:
    """The starting point: the fit on pass 1's coarse counts, on the host (a separable or degenerate set of counts ends with
    converged = False and the caller starts from where it stopped)."""
    totals(coarse)
    x, t, n = _coarse_points(coarse, lo, hi)
    S, cls, wt = np.concatenate([x, x]), np.concatenate([np.ones(len(x), np.int64), np.zeros(len(x), np.int64)]), np.concatenate([t, n])
    live = wt > 0
    S, cls, wt = S[live], cls[live], wt[live]
    # Newton starts where the scores are not saturated: the map of two Gaussians of the classes' means and the pooled variance
    mean = lambda k: float((S[cls == k] * wt[cls == k]).sum() / wt[cls == k].sum())        # noqa: E731
    m0, m1 = mean(0), mean(1)
    var = float(sum((wt[cls == k] * (S[cls == k] - m) ** 2).sum() for k, m in ((0, m0), (1, m1))) / wt.sum())
    a0 = (m1 - m0) / var if var > 0.0 and m1 > m0 else (1.0 / math.sqrt(var) if var > 0.0 else 1.0)
    return newton_fit(lambda a, c: calib_sums_host(S, cls, a, c, wt), a0, -a0 * (m0 + m1) / 2.0, prior, grad_tol, max_passes)


def pav_min_cllr(coarse: PassCounts) -> float:
    """The minimum Cllr of the coarsely quantised score: pool-adjacent-violators over the 4098 cells of pass 1 in score order (under, the
    bins, over; empty cells skipped), exact integer comparisons; a pooled block with T_g targets and N_g nontargets has the
    log-likelihood ratio ln(T_g Nn / (N_g T)).  ValueError when either class is empty."""
    T, Nn = totals(coarse)
    t = [int(coarse.under[1])] + _ints(coarse.hist[1]) + [int(coarse.over[1])]
    n = [int(coarse.under[0])] + _ints(coarse.hist[0]) + [int(coarse.over[0])]
    blocks = []                                              # (targets, trials), the target fraction non-decreasing along the stack
    for tg, ng in zip(t, n):
        if tg + ng == 0:
            continue
        ct, cn = tg, tg + ng
        while blocks and blocks[-1][0] * cn > ct * blocks[-1][1]:
            pt, pn = blocks.pop()
            ct, cn = ct + pt, cn + pn
        blocks.append((ct, cn))
    ct_sum = cn_sum = 0.0
    for tg, tot in blocks:
        ng = tot - tg
        if tg:
            ct_sum += tg * math.log1p((ng * T) / (tg * Nn))          # log(1 + exp(-llr_g))
        if ng:
            cn_sum += ng * math.log1p((tg * Nn) / (ng * T))          # log(1 + exp(+llr_g))
    return (ct_sum / T + cn_sum / Nn) / (2.0 * math.log(2.0))


def threshold_q(threshold: float, lo: float, hi: float) -> int:
    """The integer threshold of a score threshold: q(threshold) as a pass forms it, 0 below the range, 2^24 at or above hi (and for NaN)."""
    t = (np.float64(threshold) - np.float64(lo)) * np.float64(scale_of(lo, hi))
    if t != t or t >= float(Q_MAX):
        return Q_MAX
    return 0 if t < 0.0 else int(math.floor(t))


def dcf_at(coarse: PassCounts, zoom: Callable[[int], PassCounts], tq: int, p_target: float, c_miss: float, c_fa: float) -> float:
    """The normalised DCF of accepting q >= tq, exact: from pass 1 when tq is a coarse threshold, else with one zoom."""
    T, Nn = totals(coarse)
    b, j = divmod(int(tq), BINS)
    if j == 0:
        miss, fa = _cumulative(coarse)
        return _dcf(miss[b], fa[b], T, Nn, float(p_target), float(c_miss), float(c_fa))
    fine = zoom(b)
    _check_zoom(coarse, fine, b)
    fmiss, ffa = _cumulative(fine)
    return _dcf(fmiss[j], ffa[j], T, Nn, float(p_target), float(c_miss), float(c_fa))


@dataclass
class Calibration:
    kind: str
    a: float
    b: float
    prior: float                                         # the effective prior P of the fit
    score_range: Tuple[float, float]
    cllr_raw: float = math.nan
    cllr: float = math.nan
    min_cllr_coarse: float = math.nan
    bayes_threshold: float = math.nan
    act_dcf: float = math.nan
    min_dcf: float = math.nan
    n_target: int = 0
    n_nontarget: int = 0
    n_nonfinite: int = 0
    n_excluded: int = 0
    n_passes: int = 0
    converged: bool = False
    grad: Tuple[float, float] = (math.nan, math.nan)
    p_target: float = 0.01
    c_miss: float = 1.0
    c_fa: float = 1.0

    def llr(self, score):
        """a * score + b in float64."""
        return np.float64(self.a) * np.float64(score) + np.float64(self.b)


def calibration_from_passes(coarse: PassCounts, zoom: Callable[[int], PassCounts], sums: Callable[[float, float], CalibSums], kind: str, lo: float,
                            hi: float, p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0, grad_tol: float = 1e-10,
                            max_passes: int = 24, max_refine: int = 8) -> Calibration:
    """The fit and every reported value of the rule from pass 1, a zoom callback and a calibration-pass callback sums(a, c)."""
    done: Dict[int, PassCounts] = {}

    def cached(b: int) -> PassCounts:
        if b not in done:
            done[b] = zoom(b)
        return done[b]

    calls = [0]

    def counted(a: float, c: float) -> CalibSums:
        calls[0] += 1
        return sums(a, c)

    totals(coarse)
    prior = effective_prior(p_target, c_miss, c_fa)
    theta = math.log(prior / (1.0 - prior))
    raw = counted(1.0, 0.0)
    cllr_raw = cllr_of(raw)
    start = fit_from_counts(coarse, lo, hi, prior)
    a0, b0 = (start.a, start.b) if math.isfinite(start.a) and math.isfinite(start.b) and start.a > 0.0 else (1.0, 0.0)
    fit = newton_fit(counted, a0, b0, prior, grad_tol, max_passes)
    final = counted(fit.a, fit.b)
    thr = (-theta - fit.b) / fit.a if fit.a != 0.0 else math.nan
    act = dcf_at(coarse, cached, threshold_q(thr, lo, hi), p_target, c_miss, c_fa)
    d = min_dcf_from_counts(coarse, cached, lo, hi, p_target, c_miss, c_fa, max_refine)
    return Calibration(kind=kind, a=fit.a, b=fit.b, prior=prior, score_range=(float(lo), float(hi)), cllr_raw=cllr_raw, cllr=cllr_of(final),
                       min_cllr_coarse=pav_min_cllr(coarse), bayes_threshold=thr, act_dcf=act, min_dcf=d["min_dcf"], n_target=int(final.n[1]),
                       n_nontarget=int(final.n[0]), n_nonfinite=int(final.nonfinite.sum()), n_excluded=int(final.excluded), n_passes=calls[0],
                       converged=fit.converged, grad=fit.grad, p_target=float(p_target), c_miss=float(c_miss), c_fa=float(c_fa))


def sums_to_host(dev) -> CalibSums:
    """ops_score.trial_calib's device tensors -> CalibSums (this is where the host waits for the pass)."""
    n, sums, nonfinite, excluded = (t.cpu().numpy() for t in dev)
    return CalibSums(n.astype(np.int64), sums.astype(np.float64), nonfinite.astype(np.int64), int(excluded[0]))


def calibrate_scores(engine, A, B, r, la, sa, lb, sb, kind: str, score_range: Optional[Tuple[float, float]] = None, p_target: float = 0.01,
                     c_miss: float = 1.0, c_fa: float = 1.0, grad_tol: float = 1e-10, max_passes: int = 24, max_refine: int = 8,
                     max_blocks: int = 0) -> Calibration:
    """The calibration of trials already in matrix form (device tensors as Engine.trial_hist takes them), beside evaluate_scores: pass 1 and
    the zooms through Engine.trial_hist, the calibration passes through ops_score.trial_calib."""
    if kind not in ("cosine", "plda"):
        raise ValueError(f"calibrate: kind={kind!r} ('cosine' or 'plda')")
    from .ops_score import trial_calib
    lo, hi = score_range if score_range is not None else (COSINE_RANGE if kind == "cosine" else PLDA_RANGE)
    scale_of(lo, hi)

    def run(shift: int, base: int) -> PassCounts:
        return counts_to_host(engine.trial_hist(A, B, r, la, sa, lb, sb, lo, hi, shift=shift, base=base, max_blocks=max_blocks))

    return calibration_from_passes(run(COARSE_SHIFT, 0), lambda b: run(0, BINS * b),
                                   lambda a, c: sums_to_host(trial_calib(engine, A, B, r, la, sa, lb, sb, a, c, max_blocks=max_blocks)), kind, lo, hi,
                                   p_target, c_miss, c_fa, grad_tol, max_passes, max_refine)


CALIBRATION_KEYS = ("kind", "a", "b", "prior", "score_range", "cllr_raw", "cllr", "min_cllr_coarse", "bayes_threshold", "act_dcf", "min_dcf",
                    "n_target", "n_nontarget", "n_nonfinite", "n_excluded", "n_passes", "converged", "grad", "p_target", "c_miss", "c_fa")


def save_calibration(cal: Calibration, path) -> None:
    """A small JSON file of settings: every field of the Calibration, in standard JSON - a figure that is not finite (one never computed,
    or of a fit that did not converge) is written as null and read back as NaN.  Refused (ValueError): what load_calibration refuses."""
    import json
    _check_map(path, cal.kind, float(cal.a), float(cal.b), float(cal.prior), tuple(float(v) for v in cal.score_range))
    num = lambda v: float(v) if math.isfinite(float(v)) else None        # noqa: E731
    doc: Dict[str, Any] = {}
    for k in CALIBRATION_KEYS:
        v = getattr(cal, k)
        if k in ("score_range", "grad"):
            doc[k] = [num(x) for x in v]
        elif isinstance(v, (bool, np.bool_)):
            doc[k] = bool(v)
        elif isinstance(v, (int, np.integer)):
            doc[k] = int(v)
        elif isinstance(v, (float, np.floating)):
            doc[k] = num(v)
        else:
            doc[k] = v
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, allow_nan=False)
        f.write("\n")


def _check_map(path, kind, a: float, b: float, prior: float, score_range) -> None:
    """What save_calibration and load_calibration refuse in the settings that are applied."""
    if kind not in ("cosine", "plda"):
        raise ValueError(f"{path}: kind={kind!r} ('cosine' or 'plda')")
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError(f"{path}: a={a}, b={b}: the map llr = a s + b needs finite numbers")
    if a <= 0.0:
        raise ValueError(f"{path}: a={a}: a calibration keeps the order of the scores, a > 0")
    if not 0.0 < prior < 1.0:
        raise ValueError(f"{path}: prior={prior}: the effective prior of the fit lies inside (0, 1)")
    scale_of(*score_range)                                   # finite lo < hi


def load_calibration(path) -> Calibration:
    """save_calibration's file -> Calibration.  Refused (ValueError): a file that is not a JSON object with kind, a, b, prior and score_range,
    an unknown kind, an a or b that is not finite, a <= 0, a prior outside (0, 1), a score_range that is not finite lo < hi.  A null
    among the reported figures reads as NaN."""
    import json
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or any(k not in doc for k in ("kind", "a", "b", "prior", "score_range")):
        raise ValueError(f"{path}: not a calibration file (a JSON object with kind, a, b, prior, score_range: trials.save_calibration writes one)")
    try:
        a, b, prior = float(doc["a"]), float(doc["b"]), float(doc["prior"])
        lo, hi = (float(v) for v in doc["score_range"])
    except (TypeError, ValueError):
        raise ValueError(f"{path}: a, b, prior and the two ends of score_range must be numbers") from None
    _check_map(path, doc["kind"], a, b, prior, (lo, hi))
    nan = lambda v: math.nan if v is None else v                          # noqa: E731
    rest = {k: nan(doc[k]) for k in CALIBRATION_KEYS if k in doc and k not in ("kind", "a", "b", "prior", "score_range", "grad")}
    grad = tuple(float(nan(v)) for v in doc["grad"]) if "grad" in doc else (math.nan, math.nan)
    return Calibration(kind=doc["kind"], a=a, b=b, prior=prior, score_range=(lo, hi), grad=grad, **rest)


def calibrate(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, kind: str = "cosine", plda=None, count_by_book: bool = True,
              score_range: Optional[Tuple[float, float]] = None, p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0,
              grad_tol: float = 1e-10, max_passes: int = 24, max_refine: int = 8, max_blocks: int = 0) -> Calibration:
    """evaluate's trials (the same arguments, the same matrices: trial_tensors) -> their Calibration."""
    tensors = trial_tensors(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, kind, plda, count_by_book)
    return calibrate_scores(engine, *tensors, kind, score_range, p_target, c_miss, c_fa, grad_tol, max_passes, max_refine, max_blocks)


def summary(res: VerificationResult) -> Dict[str, Any]:
    """The dict Backend.tune_verification and tune_cohort_threshold answer with: a VerificationResult's figures by name, and itself."""
    return {"kind": res.kind, "eer": res.eer, "eer_threshold": res.eer_threshold, "min_dcf": res.min_dcf, "min_dcf_threshold": res.min_dcf_threshold,
            "min_dcf_lower": res.min_dcf_lower, "min_dcf_exact": res.min_dcf_exact, "n_target": res.n_target, "n_nontarget": res.n_nontarget,
            "n_nan": res.n_nan, "n_excluded": res.n_excluded, "n_test_rows": res.test_rows, "n_model_rows": res.model_rows, "score_range": res.score_range,
            "result": res}


def calibrate_verification(be: Backend, audio_paths, speaker_ids, candidates, out_path=None, score_range=None, p_target: float = 0.01,
                           c_miss: float = 1.0, c_fa: float = 1.0, grad_tol: float = 1e-10, max_passes: int = 24, max_refine: int = 8):
    """What a score of Backend `be`'s decision rule means, on a labelled development set (the arguments and the trials of
    Backend.score_verification) -> trials.Calibration: the affine map llr = a * score + b fitted by prior-weighted logistic regression on the
    device, Cllr before and after, the actual DCF at the Bayes threshold beside minDCF (trials.py states the rule; parity with outside
    toolkits is unpinned).  out_path: the calibration is also written there (trials.save_calibration), the file SDK_SCORE_CALIBRATION names.
    With a cohort configured (SDK_COHORT): ValueError - AS-norm trials are not built.  A fit that did not converge (separable classes have no
    finite minimiser): ValueError.

    A function of the Backend (backend.py, which imports it: backend.calibrate_verification), not a method of it: the Backend's public
    surface is pinned name for name (tests/test_rules_cpu.py)."""
    from . import trials
    eng, tensors, kind = be._verification_trials("calibrate_verification", audio_paths, speaker_ids, candidates)
    cal = trials.calibrate_scores(eng, *tensors, kind, score_range, p_target, c_miss, c_fa, grad_tol, max_passes, max_refine)
    if not cal.converged:
        raise ValueError(f"calibrate_verification: the fit did not converge in {cal.n_passes} passes (a={cal.a:g}, b={cal.b:g}, gradient {cal.grad}): "
                         "classes that a threshold separates without error have no finite minimiser - use more, or harder, development trials")
    if out_path is not None:
        trials.save_calibration(cal, out_path)
    return cal
