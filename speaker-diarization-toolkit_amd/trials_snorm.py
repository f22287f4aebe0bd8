"""Verification trials on the cohort-normalised (AS-norm) scale: the equal error rate, the minimum detection cost, the DET curve and the
thresholds of the Snorm decision rule (rules.py) from a labelled set of embeddings and a cohort - what SDK_COHORT_THRESHOLD is tuned with.

The rule (this build's statement; parity with any outside toolkit is unpinned, as for trials.py and snorm.py).  Trials, classes, exclusions,
the integer score q, a pass (shift, base), the counters and every metric are exactly those of trials.py.  Only the score changes:

  inputs   float64 A [N, K] and B [M, K] (K a multiple of 16 in 16 .. 512, 1 <= N, M <= 2^20) and per row two float64 statistics:
           mean_a, inv_a [N] and mean_b, inv_b [M] - the mean of the row's K largest cohort cosines and the RECIPROCAL of their standard
           deviation.
  score    s = sum_k A[i, k] B[j, k]                                              the product of trials.py without r
           z = ((s - mean_a[i]) * inv_a[i] + (s - mean_b[j]) * inv_b[j]) * 0.5
           Each operation is ONE rounded float64 operation, in this order: subtract, multiply, subtract, multiply, add, multiply by 0.5
           (never an FMA).  t = (z - lo) * scale is then formed from z as trials.py forms it from s; a NaN z is counted in nan[class].
  inv      inv = 1.0 / std is ONE float64 division per row, done by the caller on the fp32 std of Engine.cohort_stats widened to float64
           (`reciprocals`).  That std is already floored at snorm.STD_FLOOR, so inv is finite.  The kernel takes reciprocals so that a trial
           costs no division: z is snorm.py's z with `/ std` replaced by `* inv` - the two differ by the rounding of one reciprocal per
           side (a relative 2^-52 of each half of z), and by nothing else.

SNORM_RANGE = (-64, 64) is the default score range: a resolution of 128 / 2^24 = 7.6e-6 on the z scale.  Trials outside it are still
counted exactly, in under / over; an EER that falls outside raises trials.py's "wider range" error.

On the device: ops_score.trial_hist_snorm (csrc/trials_snorm.hip: trial_hist's tiling and product at width K, the normalisation in the
product's epilogue on the accumulator registers; neither matrix is written; integer counting only after z - bit-identical run to run).
This module holds the numpy restatement of a pass, operation for operation, and the driver of pass 1 and the zooms; like trials.py it imports
neither torch nor the library at module level.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, Any, Dict, Optional, Tuple

import numpy as np

from . import trials
from .trials import BINS, COARSE_SHIFT, PassCounts, VerificationResult

if TYPE_CHECKING:
    from .backend import Backend

SNORM_RANGE = (-64.0, 64.0)
STATS_BLOCK = 65536                # rows per Engine.cohort_stats call


def snorm_scores_host(A, B, mean_a, inv_a, mean_b, inv_b) -> np.ndarray:
    """z [N, M] in numpy float64, operation for operation as the kernel's epilogue forms it (numpy rounds every elementwise operation)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ma, ia, mb, ib = (np.asarray(v, dtype=np.float64) for v in (mean_a, inv_a, mean_b, inv_b))
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError(f"trial_hist_snorm_host: A {A.shape} and B {B.shape} do not belong together")
    if ma.shape != (A.shape[0],) or ia.shape != (A.shape[0],) or mb.shape != (B.shape[0],) or ib.shape != (B.shape[0],):
        raise ValueError(f"trial_hist_snorm_host: one mean and one inv per row expected: mean_a {ma.shape}, inv_a {ia.shape} for {A.shape[0]} test "
                         f"rows, mean_b {mb.shape}, inv_b {ib.shape} for {B.shape[0]} model rows")
    with np.errstate(invalid="ignore", over="ignore"):
        S = A @ B.T
        za = (S - ma[:, None]) * ia[:, None]
        zb = (S - mb[None, :]) * ib[None, :]
        return (za + zb) * np.float64(0.5)


def trial_hist_snorm_host(A, B, mean_a, inv_a, mean_b, inv_b, la, sa, lb, sb, lo: float, hi: float, shift: int = COARSE_SHIFT,
                          base: int = 0) -> PassCounts:
    """The numpy restatement of ops_score.trial_hist_snorm: z, then one pass of trials.py."""
    Z = snorm_scores_host(A, B, mean_a, inv_a, mean_b, inv_b)
    la, sa, lb, sb = (np.asarray(v) for v in (la, sa, lb, sb))
    if la.shape != (Z.shape[0],) or sa.shape != (Z.shape[0],) or lb.shape != (Z.shape[1],) or sb.shape != (Z.shape[1],):
        raise ValueError(f"trial_hist_snorm_host: one label and one session per row expected: la {la.shape}, sa {sa.shape} for {Z.shape[0]} test "
                         f"rows, lb {lb.shape}, sb {sb.shape} for {Z.shape[1]} model rows")
    return trials.counts_from_scores(Z, trials.trial_classes(la, sa, lb, sb), lo, hi, shift, base)


def reciprocals(std):
    """The fp32 std of Engine.cohort_stats (a device tensor, floored at snorm.STD_FLOOR) -> inv = 1.0 / float64(std): one float64 division
    per row."""
    return (1.0 / std.double()).contiguous()


def cohort_statistics(engine, E, cohort_rows, topk: int):
    """(mean [N], inv [N]) float64 device tensors of the unit fp32 rows E [N, d]: Engine.cohort_stats in blocks of at most 65 536 rows,
    widened, the standard deviation inverted (`reciprocals`)."""
    import torch
    n = int(E.shape[0])
    parts = [engine.cohort_stats(E[a:a + STATS_BLOCK], cohort_rows, topk) for a in range(0, n, STATS_BLOCK)]
    mean = parts[0][0] if len(parts) == 1 else torch.cat([p[0] for p in parts])
    std = parts[0][1] if len(parts) == 1 else torch.cat([p[1] for p in parts])
    return mean.double().contiguous(), reciprocals(std)


def evaluate_snorm_scores(engine, A, B, mean_a, inv_a, mean_b, inv_b, la, sa, lb, sb, score_range: Optional[Tuple[float, float]] = None,
                          p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0, max_refine: int = 8,
                          max_blocks: int = 0) -> VerificationResult:
    """Pass 1 and the zooms on the device for trials already in matrix form (device tensors as ops_score.trial_hist_snorm takes them)."""
    from .ops_score import trial_hist_snorm
    lo, hi = score_range if score_range is not None else SNORM_RANGE
    trials.scale_of(lo, hi)

    def run(shift: int, base: int) -> PassCounts:
        return trials.counts_to_host(trial_hist_snorm(engine, A, B, mean_a, inv_a, mean_b, inv_b, la, sa, lb, sb, lo, hi, shift=shift, base=base,
                                                      max_blocks=max_blocks))

    coarse = run(COARSE_SHIFT, 0)
    res = trials.result_from_passes(coarse, lambda b: run(0, BINS * b), "snorm", lo, hi, p_target, c_miss, c_fa, max_refine)
    res.test_rows, res.model_rows = int(A.shape[0]), int(B.shape[0])
    return res


def evaluate_snorm(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, cohort_rows, topk, score_range=None,
                   p_target: float = 0.01, c_miss: float = 1.0, c_fa: float = 1.0, max_refine: int = 8, max_blocks: int = 0) -> VerificationResult:
    """Every test row against every model row on the AS-norm scale -> trials.VerificationResult with kind="snorm".  E_test [N, d], E_model
    [P, d] and their labels and sessions: as trials.evaluate takes them under the cosine rule (the model rows are scored one by one).
    cohort_rows [C, d]: the cohort's unit fp32 rows on the device (snorm.Cohort.device_rows); topk: the cohort scores per row that the
    statistics are taken over, 1 .. C.  Engine.cohort_stats runs on both sides; score_range defaults to SNORM_RANGE."""
    if cohort_rows is None:
        raise ValueError("evaluate_snorm: no cohort: cohort_rows (the cohort's unit fp32 rows on the device, snorm.Cohort.device_rows) is None")
    if topk is None:
        raise ValueError("evaluate_snorm: topk is None (the cohort scores per row that the statistics are taken over, 1 .. the cohort's rows)")
    A, B, _, la, sa, lb, sb = trials.trial_tensors(engine, E_test, labels, sessions, E_model, model_labels, model_sessions, "cosine")
    mean_a, inv_a = cohort_statistics(engine, E_test.contiguous(), cohort_rows, int(topk))
    mean_b, inv_b = cohort_statistics(engine, E_model.contiguous(), cohort_rows, int(topk))
    return evaluate_snorm_scores(engine, A, B, mean_a, inv_a, mean_b, inv_b, la, sa, lb, sb, score_range, p_target, c_miss, c_fa, max_refine,
                                 max_blocks)


# ---- the trials of a Backend (backend.py).  Functions of it, not methods: its public surface is pinned name for name
#      (tests/test_rules_cpu.py); backend.py imports them, so callers reach them as backend.tune_cohort_threshold and so on.
def _snorm_trials(be: Backend, who: str, audio_paths, speaker_ids, candidates, cohort, topk, score_range, p_target, c_miss, c_fa, max_refine):
    """-> (trials.VerificationResult, the snorm.Cohort, the K its statistics were taken over)."""
    from . import trials_snorm
    from .rules import Cosine
    from .snorm import Cohort
    if be.lite:
        raise ValueError(f"{who}: needs the torch engine; unset SDK_NO_TORCH")
    co = be.cohort() if cohort is None else cohort if isinstance(cohort, Cohort) else Cohort.load(cohort, be.embedding_dim)
    if co is None:
        raise ValueError(f"{who}: no cohort: pass cohort= (a .npy path as SDK_COHORT names one, Backend.make_cohort writes it; or a snorm.Cohort) "
                         "or configure SDK_COHORT")
    if co.dim != int(be.embedding_dim):
        raise ValueError(f"{who}: cohort {co.source}: rows of d={co.dim}, the model's embedding_dim is {int(be.embedding_dim)}")
    K = min(int(be.cohort_topk if topk is None else topk), len(co))
    if K < 1:
        raise ValueError(f"{who}: topk={topk}: at least 1")
    eng, E, speaker_ids, counts, batch = be._trial_windows(who, audio_paths, speaker_ids, candidates)
    A, B, _, lb, _, index = Cosine().trial_matrices(be, E, batch)              # the cosine rule's matrices: windows against enrolled embeddings
    la, sa, lb, sb = be._trial_labels(E.device, speaker_ids, counts, lb, index)
    rows = co.device_rows(eng)
    mean_a, inv_a = trials_snorm.cohort_statistics(eng, E, rows, K)
    mean_b, inv_b = trials_snorm.cohort_statistics(eng, be.profile_tensors(batch)[0].contiguous(), rows, K)
    res = trials_snorm.evaluate_snorm_scores(eng, A, B, mean_a, inv_a, mean_b, inv_b, la, sa, lb, sb, score_range, p_target, c_miss, c_fa, max_refine)
    return res, co, K


def score_verification_snorm(be: Backend, audio_paths, speaker_ids, candidates, cohort=None, topk=None, score_range=None, p_target: float = 0.01,
                             c_miss: float = 1.0, c_fa: float = 1.0, max_refine: int = 8):
    """Backend.score_verification on the AS-norm scale -> trials.VerificationResult with kind "snorm": how well the cohort-normalised decision
    of identify_speaker / verify_speaker (SDK_COHORT) separates the enrolled speakers on labelled recordings.  The inputs and the trials are
    those of Backend.score_verification under the cosine rule: every window of every recording is a test row, the model rows are the
    candidates' enrolled embeddings (profile_tensors).  cohort: a .npy path (Backend.make_cohort writes one) or a snorm.Cohort; None: the
    configured SDK_COHORT (ValueError when neither is given).  topk: the cohort scores per side that the statistics are taken over; None:
    the backend's cohort_topk (SDK_COHORT_TOPK); min(topk, the cohort's rows) is used.  score_range defaults to trials_snorm.SNORM_RANGE.
    Works on a Backend under the cosine rule and on one configured with SDK_COHORT; SDK_NO_TORCH=1 is refused.  trials_snorm.py states
    the rule (parity with outside toolkits is unpinned).

    A function of the Backend (backend.py, which imports it: backend.score_verification_snorm), not a method of it: the Backend's public
    surface is pinned name for name (tests/test_rules_cpu.py)."""
    return _snorm_trials(be, "score_verification_snorm", audio_paths, speaker_ids, candidates, cohort, topk, score_range, p_target, c_miss, c_fa,
                         max_refine)[0]


def tune_cohort_threshold(be: Backend, audio_paths, speaker_ids, candidates, cohort=None, topk=None, score_range=None, p_target: float = 0.01,
                          c_miss: float = 1.0, c_fa: float = 1.0, max_refine: int = 8) -> Dict[str, Any]:
    """The thresholds of the AS-norm decision on a labelled development set (the arguments of score_verification_snorm) ->
    Backend.tune_verification's dict with kind "snorm", plus "cohort_digest" (the content hash of the cohort the statistics came from) and
    "topk" (the K used).  eer_threshold and min_dcf_threshold are on the z scale: they are what SDK_COHORT_THRESHOLD takes, for THIS cohort
    and K.  The evaluation scores the float64 product of the fp32 unit rows and normalises it in float64; identify computes z from its
    fp32 cosines and fp32 statistics.  The two agree to fp32 rounding times inv = 1 / std (a few 1e-7 of cosine, scaled by 1 / std), so
    a window that close to the threshold may vote differently."""
    res, co, K = _snorm_trials(be, "tune_cohort_threshold", audio_paths, speaker_ids, candidates, cohort, topk, score_range, p_target, c_miss, c_fa,
                               max_refine)
    return dict(trials.summary(res), cohort_digest=co.digest, topk=K)
