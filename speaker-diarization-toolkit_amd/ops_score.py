"""Engine's scoring calls beyond the cosine affinity: adaptive score normalisation against a cohort (snorm.py), the PLDA's training
statistics and projection (plda.fit), PLDA log-likelihood-ratio scoring (plda_score.py), the verification-trial histogram and calibration
pass (trials.py), the histogram on the cohort-normalised scale (trials_snorm.py) and the attribution of a transcript's words to the
diarization's frames (words.py) and each speaker's solo runs and clip scores (samples.py).  Nothing here synchronises with the host except
plda_fit_stats' range check of its labels.

ScoreMixin is a mixin of ops.Engine: no state and no __init__ of its own.  It uses self.lib, self.ctx, self.device, self._workspace
only, and this module imports ops.py for nothing (ops.py imports it).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _args
from ._lib import check
from .ops_util import _ptr, _stream


class ScoreMixin:
    # ------------------------------------------------------------------ adaptive score normalisation (snorm.py; csrc/snorm.hip)
    def cohort_stats(self, E: torch.Tensor, cohort: torch.Tensor, K: int, ws: Optional[torch.Tensor] = None):
        """Unit fp32 rows E [N, d] and cohort [M, d] (device) -> (mean [N], std [N]) fp32 of every row's K largest cohort cosines: the mean and
        the population standard deviation, floored at snorm.STD_FLOOR (sdk_cohort_stats).  ws: a uint8 device tensor to use as the workspace
        (default: one of sdk_cohort_stats_workspace_bytes(N, M, K) bytes is allocated)."""
        N, d = _args.rows("cohort_stats", "E", E)
        M, _ = _args.rows("cohort_stats", "the cohort", cohort, d=d)
        K = int(K)
        if M < 1 or M > (1 << 20):
            raise ValueError(f"cohort_stats: M={M} cohort rows (1 .. 2^20)")
        if K < 1 or K > M:
            raise ValueError(f"cohort_stats: K={K} (1 .. M={M})")
        ws = self._workspace("sdk_cohort_stats_workspace_bytes", N, M, K) if ws is None else _args.tensor("cohort_stats", "ws", ws, "uint8", (None,))
        mean = torch.empty((N,), dtype=torch.float32, device=E.device)
        std = torch.empty((N,), dtype=torch.float32, device=E.device)
        check(self.lib.sdk_cohort_stats(self.ctx, E.data_ptr(), N, cohort.data_ptr(), M, d, K, mean.data_ptr(), std.data_ptr(), ws.data_ptr(),
                                        ws.numel(), _stream()), "sdk_cohort_stats")
        return mean, std

    def affinity_topk_snorm(self, E: torch.Tensor, mean_e: torch.Tensor, std_e: torch.Tensor, P: torch.Tensor, mean_p: torch.Tensor,
                            std_p: torch.Tensor, k: int = 1):
        """Unit fp32 rows E [N, d] and P [Pn, d] with their cohort statistics (cohort_stats) -> (idx [N, k] int32, score [N, k] fp32,
        raw [N, k] fp32): per window the k <= min(4, Pn) largest z = ((s - mean_e) / std_e + (s - mean_p) / std_p) / 2, s the cosine; ties to
        the lower profile; raw is s.  A slot without a finite z holds (-1, 0, 0) (sdk_affinity_topk_snorm)."""
        who = "affinity_topk_snorm"
        N, d = _args.rows(who, "E", E)
        Pn, _ = _args.rows(who, "P", P, d=d)
        for name, t, n in (("mean_e", mean_e, N), ("std_e", std_e, N), ("mean_p", mean_p, Pn), ("std_p", std_p, Pn)):
            _args.tensor(who, name, t, "float32", (n,))
        k = int(k)
        if k < 1 or k > 4:
            raise ValueError(f"affinity_topk_snorm: k={k} (1 .. 4)")
        if Pn < 1 or k > Pn:
            raise ValueError(f"affinity_topk_snorm: k={k} with Pn={Pn} profiles (the caller clamps k to the number of profiles, at least 1)")
        idx = torch.empty((N, k), dtype=torch.int32, device=E.device)
        sc = torch.empty((N, k), dtype=torch.float32, device=E.device)
        raw = torch.empty((N, k), dtype=torch.float32, device=E.device)
        check(self.lib.sdk_affinity_topk_snorm(self.ctx, E.data_ptr(), mean_e.data_ptr(), std_e.data_ptr(), N, P.data_ptr(), mean_p.data_ptr(),
                                               std_p.data_ptr(), Pn, d, k, idx.data_ptr(), sc.data_ptr(), raw.data_ptr(), _stream()),
              "sdk_affinity_topk_snorm")
        return idx, sc, raw

    # ---- training the PLDA from labelled rows (plda.fit; csrc/plda_fit.hip)
    def plda_fit_stats(self, rows: torch.Tensor, labels: Optional[torch.Tensor] = None, K: int = 0, mean1: Optional[torch.Tensor] = None,
                       scatter: bool = True, check_labels: bool = True) -> dict:
        """rows [N, d] on the device: fp32 (d a multiple of 64, at most 512; with mean1 [d] float64 every row enters as
        sqrt(d) unit(e - mean1)) or float64 as they lie (d 1 .. 512); labels [N] int32 in [0, K) or None (K = 0: the total and the scatter
        only) -> dict(counts [K] int64, sums [K, d], total [d], scatter [d, d] or None, status [1] int32), float64 on the device:
        sdk_plda_fit_stats.  The labels' range is checked here, before any launch (one read-back; check_labels=False: the caller has), and the
        row indices are sorted by label with torch's stable sort."""
        who = "plda_fit_stats"
        _args.tensor(who, "rows", rows, ("float32", "float64"), (None, None))
        N, d, K = int(rows.shape[0]), int(rows.shape[1]), int(K)
        f32 = rows.dtype == torch.float32
        if N < 1 or N > 1 << 24:
            raise ValueError(f"plda_fit_stats: N={N} rows (1 .. 2^24)")
        if f32:
            _args.row_width(who, d)
        elif d < 1 or d > _args.MAX_ROW_DIM:
            raise ValueError(f"plda_fit_stats: d={d} not supported (float64 rows: 1 .. {_args.MAX_ROW_DIM})")
        if mean1 is not None:
            if not f32:
                raise ValueError("plda_fit_stats: mean1 goes with fp32 rows")
            _args.tensor(who, "mean1", mean1, "float64", (d,))
        if K < 0 or K > 1 << 24 or (labels is None) != (K == 0):
            raise ValueError(f"plda_fit_stats: K={K} (1 .. 2^24 with labels, 0 without)")
        dev = rows.device
        order = counts = sums = None
        if labels is not None:
            _args.tensor(who, "labels", labels, "int32", (N,))
            if check_labels:
                lo, hi = int(labels.min()), int(labels.max())
                if lo < 0 or hi >= K:
                    raise ValueError(f"plda_fit_stats: labels must lie in [0, {K}), got {lo} .. {hi}")
            order = torch.sort(labels, stable=True).indices.to(torch.int32)
            counts = torch.empty((K,), dtype=torch.int64, device=dev)
            sums = torch.empty((K, d), dtype=torch.float64, device=dev)
        ws = self._workspace("sdk_plda_fit_stats_workspace_bytes", N, d, K, int(bool(scatter)))
        total = torch.empty((d,), dtype=torch.float64, device=dev)
        S = torch.empty((d, d), dtype=torch.float64, device=dev) if scatter else None
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        check(self.lib.sdk_plda_fit_stats(self.ctx, rows.data_ptr() if f32 else None, None if f32 else rows.data_ptr(), _ptr(mean1), N, d, _ptr(labels),
                                          _ptr(order), K, _ptr(counts), _ptr(sums), total.data_ptr(), _ptr(S), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _stream()), "sdk_plda_fit_stats")
        return dict(counts=counts, sums=sums, total=total, scatter=S, status=status)

    def plda_project(self, E: torch.Tensor, mean1: torch.Tensor, lda: torch.Tensor, mean2: torch.Tensor) -> torch.Tensor:
        """E [N, d_in] fp32 rows, mean1 [d_in], lda [d_in, D0], mean2 [D0] (float64, device) -> x2 [N, D0] float64:
        sqrt(D0) unit(lda^T sqrt(d_in) unit(e - mean1) - mean2), sdk_plda_transform's first two steps for every row (sdk_plda_project)."""
        who = "plda_project"
        N, d_in = _args.rows(who, "E", E)
        if N < 1 or N > 1 << 24:
            raise ValueError(f"plda_project: N={N} rows (1 .. 2^24)")
        D0 = int(_args.tensor(who, "lda", lda, "float64", (d_in, None)).shape[1])
        if not 1 <= D0 <= _args.MAX_ROW_DIM:
            raise ValueError(f"plda_project: lda must be [{d_in}, D0 <= {_args.MAX_ROW_DIM}], got {list(lda.shape)}")
        _args.tensor(who, "mean1", mean1, "float64", (d_in,))
        _args.tensor(who, "mean2", mean2, "float64", (D0,))
        X2 = torch.empty((N, D0), dtype=torch.float64, device=E.device)
        check(self.lib.sdk_plda_project(self.ctx, E.data_ptr(), d_in, N, mean1.data_ptr(), lda.data_ptr(), mean2.data_ptr(), D0, X2.data_ptr(),
                                        _stream()), "sdk_plda_project")
        return X2

    # ---- PLDA log-likelihood-ratio scoring (plda_score.py; csrc/plda_score.hip)
    def plda_enroll(self, Xp: torch.Tensor, group: torch.Tensor, n_eff: torch.Tensor, Phi: torch.Tensor):
        """Xp [P, D] float64 transformed profile rows (plda_transform; D 64 or 128, P <= 2^22), group [P] int32 (the speaker index of every
        row, in any order), n_eff [S] float64 (1 <= S <= 2^20), Phi [D] float64, all on the device -> (G [S, 2 D], r [S], status [1] int32)
        on the device: the speaker table of plda_score.py (sdk_plda_enroll).  A label outside [0, S) belongs to no speaker and sets status
        bit 1; a speaker without a row or with an n_eff that is not a finite number above 0 gets r = NaN.  The caller reads status."""
        who = "plda_enroll"
        P, D = (int(v) for v in _args.tensor(who, "Xp", Xp, "float64", (None, None)).shape)
        if D not in (64, 128):
            raise ValueError(f"plda_enroll: D={D} not supported (64 or 128)")
        if P > 1 << 22:
            raise ValueError(f"plda_enroll: P={P} rows (0 .. 2^22)")
        _args.tensor(who, "group", group, "int32", (P,))
        S = int(_args.tensor(who, "n_eff", n_eff, "float64", (None,)).shape[0])
        if S < 1 or S > 1 << 20:
            raise ValueError(f"plda_enroll: S={S} speakers (1 .. 2^20)")
        _args.tensor(who, "Phi", Phi, "float64", (D,))
        ws = self._workspace("sdk_plda_enroll_workspace_bytes", P, S)
        dev = Xp.device
        G = torch.empty((S, 2 * D), dtype=torch.float64, device=dev)
        r = torch.empty((S,), dtype=torch.float64, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        check(self.lib.sdk_plda_enroll(self.ctx, Xp.data_ptr() if P else None, group.data_ptr() if P else None, P, D, n_eff.data_ptr(),
                                       Phi.data_ptr(), S, G.data_ptr(), r.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "sdk_plda_enroll")
        return G, r, status

    def plda_score_topk(self, X: torch.Tensor, G: torch.Tensor, r: torch.Tensor, k: int = 1, scores: bool = False,
                        ws: Optional[torch.Tensor] = None):
        """X [N, D] float64 transformed windows (N <= 65 536), (G [S, 2 D], r [S]) a speaker table of plda_enroll -> (idx [N, k] int32,
        score [N, k] float64) and, with scores=True, the whole matrix [N, S]: per window the k <= 4 largest log-likelihood ratios
        r_s + sum_d x_d G[s, d] + x_d^2 G[s, D + d]; ties to the lower speaker, a NaN never taken, a slot without a candidate holds
        (-1, 0); with k > S the columns S .. k - 1 are not written (sdk_plda_score_topk).  ws: a uint8 device tensor to use as the workspace
        (default: one of sdk_plda_score_workspace_bytes(N, S, k) bytes is allocated)."""
        who = "plda_score_topk"
        N, D = (int(v) for v in _args.tensor(who, "X", X, "float64", (None, None)).shape)
        if D not in (64, 128):
            raise ValueError(f"plda_score_topk: D={D} not supported (64 or 128)")
        if N > 65536:
            raise ValueError(f"plda_score_topk: N={N} windows (0 .. 65536)")
        S, k = int(_args.tensor(who, "G", G, "float64", (None, 2 * D)).shape[0]), int(k)
        if S < 1 or S > 1 << 20:
            raise ValueError(f"plda_score_topk: S={S} speakers (1 .. 2^20)")
        _args.tensor(who, "r", r, "float64", (S,))
        if k < 1 or k > 4:
            raise ValueError(f"plda_score_topk: k={k} (1 .. 4)")
        ws = self._workspace("sdk_plda_score_workspace_bytes", N, S, k) if ws is None else _args.tensor(who, "ws", ws, "uint8", (None,))
        dev = X.device
        idx = torch.empty((N, k), dtype=torch.int32, device=dev)
        sc = torch.empty((N, k), dtype=torch.float64, device=dev)
        full = torch.empty((N, S), dtype=torch.float64, device=dev) if scores else None
        check(self.lib.sdk_plda_score_topk(self.ctx, X.data_ptr(), N, D, G.data_ptr(), r.data_ptr(), S, k, idx.data_ptr(), sc.data_ptr(), _ptr(full),
                                           ws.data_ptr(), ws.numel(), _stream()), "sdk_plda_score_topk")
        return (idx, sc, full) if scores else (idx, sc)

    # ---- verification trials (trials.py; csrc/trials.hip)
    def trial_hist(self, A: torch.Tensor, B: torch.Tensor, r: torch.Tensor, la: torch.Tensor, sa: torch.Tensor, lb: torch.Tensor,
                   sb: torch.Tensor, lo: float, hi: float, shift: int = 12, base: int = 0, max_blocks: int = 0):
        """One pass of the trial histogram: A [N, K] test rows, B [M, K] model rows, r [M] float64 (K a multiple of 16 in 16 .. 512,
        1 <= N, M <= 2^20), la, sa [N] and lb, sb [M] int32 labels and sessions, all on the device -> (hist [2, 4096], under [2], over [2],
        nan [2], excluded [1]) int64 device tensors, views of one array (sdk_trial_hist; trials.py states the rule).  The score
        r[j] + A[i] . B[j] is cut into q = floor((s - lo) * scale), scale = 2^24 / (hi - lo) formed here in float64, and lands in bin
        (q >> shift) - base.  max_blocks: 0 = the default grid, else a cap on the workgroups (the counts do not depend on it)."""
        N, M, K = _trial_tensors("trial_hist", A, B, (("r", r, "M"),), la, sa, lb, sb)
        lo, scale, shift, base, max_blocks = _trial_range("trial_hist", lo, hi, shift, base, max_blocks)
        out = torch.empty((_TRIAL_OUT,), dtype=torch.int64, device=A.device)             # uint64 counters, all below 2^40
        check(self.lib.sdk_trial_hist(self.ctx, A.data_ptr(), N, B.data_ptr(), r.data_ptr(), M, K, la.data_ptr(), sa.data_ptr(), lb.data_ptr(),
                                      sb.data_ptr(), lo, scale, shift, base, max_blocks, out.data_ptr(), _stream()), "sdk_trial_hist")
        return _trial_views(out)


_TRIAL_OUT = 2 * 4096 + 7      # hist[2][4096], under[2], over[2], nan[2], excluded[1] (csrc/trial_tile.hpp)


def _trial_tensors(who: str, A, B, payload, la, sa, lb, sb):
    """The tensors every trial pass takes: A [N, K], B [M, K] float64, the pass's own float64 rows `payload` ((name, tensor, "N" or "M"), ..)
    and the int32 labels and sessions -> (N, M, K)."""
    N, K = (int(v) for v in _args.tensor(who, "A", A, "float64", (None, None)).shape)
    if K < 16 or K > 512 or K % 16:
        raise ValueError(f"{who}: K={K} not supported (a multiple of 16 in 16 .. 512)")
    M = int(_args.tensor(who, "B", B, "float64", (None, K)).shape[0])
    if not (1 <= N <= 1 << 20 and 1 <= M <= 1 << 20):
        raise ValueError(f"{who}: N={N} test rows, M={M} model rows (1 .. 2^20 each)")
    for name, t, side in payload:
        _args.tensor(who, name, t, "float64", (N if side == "N" else M,))
    for name, t, n in (("la", la, N), ("sa", sa, N), ("lb", lb, M), ("sb", sb, M)):
        _args.tensor(who, name, t, "int32", (n,))
    return N, M, K


def _trial_max_blocks(who: str, max_blocks) -> int:
    max_blocks = int(max_blocks)
    if max_blocks < 0:
        raise ValueError(f"{who}: max_blocks={max_blocks} (0: the default grid, else a cap on the workgroups)")
    return max_blocks


def _trial_range(who: str, lo, hi, shift, base, max_blocks):
    """The score range of a histogram pass -> (lo, scale = 2^24 / (hi - lo) in float64, shift, base, max_blocks)."""
    lo, hi, shift, base = float(lo), float(hi), int(shift), int(base)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"{who}: score range ({lo}, {hi}): finite lo < hi expected")
    with np.errstate(over="ignore"):
        scale = float(np.float64(16777216.0) / (np.float64(hi) - np.float64(lo)))
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"{who}: scale = 2^24 / (hi - lo) = {scale} is not a finite number above 0 (range ({lo}, {hi}))")
    if shift < 0 or shift > 24:
        raise ValueError(f"{who}: shift={shift} (0 .. 24)")
    if base < 0 or base > 1 << 24:
        raise ValueError(f"{who}: base={base} (0 .. 2^24)")
    return lo, scale, shift, base, _trial_max_blocks(who, max_blocks)


def _trial_views(out: torch.Tensor):
    """(hist [2, 4096], under [2], over [2], nan [2], excluded [1]): views of a histogram pass's one array."""
    return out[:8192].view(2, 4096), out[8192:8194], out[8194:8196], out[8196:8198], out[8198:8199]


# ---- calibration of verification scores (trials.py; csrc/trials.hip)
def trial_calib(engine, A: torch.Tensor, B: torch.Tensor, r: torch.Tensor, la: torch.Tensor, sa: torch.Tensor, lb: torch.Tensor, sb: torch.Tensor,
                a: float, c: float, max_blocks: int = 0):
    """One pass of the calibration objective over the trials of Engine.trial_hist (the same tensors) at the map z = a * s + c ->
    (n [2] int64, sums [2, 7] float64, nonfinite [2] int64, excluded [1] int64) device tensors; row 0 nontarget, row 1 target; the sums are
    L, W0, W1, H0, H1, H2, S1 of trials.py (sdk_trial_calib).  Nothing waits.  max_blocks: 0 = the default grid, else a cap on the
    workgroups (the counts do not depend on it; the sums change by rounding).

    A function of the engine, not a method of it: Engine's public surface is pinned name for name (tests/test_ops_layout_cpu.py)."""
    N, M, K = _trial_tensors("trial_calib", A, B, (("r", r, "M"),), la, sa, lb, sb)
    a, c = float(a), float(c)
    if not (np.isfinite(a) and np.isfinite(c)):
        raise ValueError(f"trial_calib: a={a}, c={c} (the map z = a s + c: both finite)")
    max_blocks = _trial_max_blocks("trial_calib", max_blocks)
    ws = engine._workspace("sdk_trial_calib_workspace_bytes", N, M, max_blocks)
    sums = torch.empty((2, 7), dtype=torch.float64, device=A.device)
    counts = torch.empty((5,), dtype=torch.int64, device=A.device)                     # uint64 counters, all below 2^40
    check(engine.lib.sdk_trial_calib(engine.ctx, A.data_ptr(), N, B.data_ptr(), r.data_ptr(), M, K, la.data_ptr(), sa.data_ptr(), lb.data_ptr(),
                                     sb.data_ptr(), a, c, max_blocks, sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "sdk_trial_calib")
    return counts[0:2], sums, counts[2:4], counts[4:5]


# ---- verification trials on the cohort-normalised scale (trials_snorm.py; csrc/trials_snorm.hip)
def trial_hist_snorm(engine, A: torch.Tensor, B: torch.Tensor, mean_a: torch.Tensor, inv_a: torch.Tensor, mean_b: torch.Tensor, inv_b: torch.Tensor,
                     la: torch.Tensor, sa: torch.Tensor, lb: torch.Tensor, sb: torch.Tensor, lo: float, hi: float, shift: int = 12, base: int = 0,
                     max_blocks: int = 0):
    """One pass of the trial histogram on the AS-norm scale: Engine.trial_hist's A [N, K], B [M, K], labels and sessions (no r), and per row the
    float64 mean of its cohort scores and the RECIPROCAL of their standard deviation - mean_a, inv_a [N], mean_b, inv_b [M] - all on the
    device -> Engine.trial_hist's five int64 views (hist [2, 4096], under [2], over [2], nan [2], excluded [1]) of
    z = ((s - mean_a[i]) * inv_a[i] + (s - mean_b[j]) * inv_b[j]) * 0.5, s = A[i] . B[j], cut into q = floor((z - lo) * scale) as there
    (sdk_trial_hist_snorm; trials_snorm.py states the rule).  Nothing waits.

    A function of the engine, not a method of it: Engine's public surface is pinned name for name (tests/test_ops_layout_cpu.py)."""
    lo, scale, shift, base, max_blocks = _trial_range("trial_hist_snorm", lo, hi, shift, base, max_blocks)
    N, M, K = _trial_tensors("trial_hist_snorm", A, B, (("mean_a", mean_a, "N"), ("inv_a", inv_a, "N"), ("mean_b", mean_b, "M"), ("inv_b", inv_b, "M")),
                             la, sa, lb, sb)
    out = torch.empty((_TRIAL_OUT,), dtype=torch.int64, device=A.device)                 # uint64 counters, all below 2^40
    check(engine.lib.sdk_trial_hist_snorm(engine.ctx, A.data_ptr(), N, B.data_ptr(), M, K, mean_a.data_ptr(), inv_a.data_ptr(), mean_b.data_ptr(),
                                          inv_b.data_ptr(), la.data_ptr(), sa.data_ptr(), lb.data_ptr(), sb.data_ptr(), lo, scale, shift, base,
                                          max_blocks, out.data_ptr(), _stream()), "sdk_trial_hist_snorm")
    return _trial_views(out)


# ---- speaker-attributed transcripts (words.py; csrc/words.hip)
def _prefix(who: str, name: str, t, R: int):
    return _args.tensor(who, name, t, "int32", (R + 1,))


def words_attribute(engine, words: torch.Tensor, word_off: torch.Tensor, speakers: torch.Tensor, frame_off: torch.Tensor, cent_off: torch.Tensor,
                    max_hyp: int, gap_frames: int) -> torch.Tensor:
    """words [W, 2] int32 (s0, s1 in samples inside the word's recording), speakers [G, 2] int32 on the packed frame grid, word_off, frame_off,
    cent_off [R + 1] int32 prefix sums (diarize_ops.GroupTables), all on the device -> rows [W, 8] int32 (speaker, votes, solo, span, second,
    second_votes, distance, g0) on the device: one launch, one wave per word (sdk_words_attribute; words.py states the rule).  max_hyp: the
    largest K_r of the pack (at most words.MAX_WORD_SPEAKERS); gap_frames: how far a word in non-speech looks for a voiced frame.  Nothing waits.

    A function of the engine, not a method of it: Engine's public surface is pinned name for name (tests/test_ops_layout_cpu.py)."""
    who = "words_attribute"
    W = int(_args.tensor(who, "words", words, "int32", (None, 2)).shape[0])
    G = int(_args.tensor(who, "speakers", speakers, "int32", (None, 2)).shape[0])
    R = int(_args.tensor(who, "word_off", word_off, "int32", (None,)).shape[0]) - 1
    if R < 1:
        raise ValueError(f"words_attribute: word_off must hold R + 1 >= 2 prefix sums, got {list(word_off.shape)}")
    _prefix(who, "frame_off", frame_off, R)
    _prefix(who, "cent_off", cent_off, R)
    max_hyp, gap_frames = int(max_hyp), int(gap_frames)
    if max_hyp < 0 or max_hyp > 1024:
        raise ValueError(f"words_attribute: {max_hyp} hypothesis speakers in a recording (at most 1024)")
    if gap_frames < 0 or gap_frames >= 1 << 30:
        raise ValueError(f"words_attribute: gap_frames={gap_frames} (0 .. 2^30 - 1)")
    out = torch.empty((W, 8), dtype=torch.int32, device=words.device)
    check(engine.lib.sdk_words_attribute(engine.ctx, words.data_ptr() if W else None, word_off.data_ptr(), speakers.data_ptr() if G else None,
                                         frame_off.data_ptr(), cent_off.data_ptr(), R, W, G, max_hyp, gap_frames, out.data_ptr() if W else None,
                                         _stream()), "sdk_words_attribute")
    return out


def words_cooccur(engine, rows: torch.Tensor, ref: torch.Tensor, word_off: torch.Tensor, ref_off: torch.Tensor, cent_off: torch.Tensor,
                  co_off: torch.Tensor, max_ref: int, max_hyp: int, co_total: int):
    """rows [W, 8] int32 (words_attribute), ref [W] int32 (the reference speaker of every word, -1: not scored), word_off, ref_off, cent_off
    [R + 1] int32 and co_off [R + 1] int64 prefix sums, all on the device -> (co [max(co_total, 1)] int32: recording r's [S_r, K_r] table at co_off[r];
    tally [R, 3] int64: scored, unassigned, words) on the device (sdk_words_cooccur); Engine.score_map's kernel then runs on co.  At most 64
    speakers a side.  Nothing waits.

    A function of the engine, not a method of it: Engine's public surface is pinned name for name (tests/test_ops_layout_cpu.py)."""
    who = "words_cooccur"
    W = int(_args.tensor(who, "rows", rows, "int32", (None, 8)).shape[0])
    _args.tensor(who, "ref", ref, "int32", (W,))
    R = int(_args.tensor(who, "word_off", word_off, "int32", (None,)).shape[0]) - 1
    if R < 1:
        raise ValueError(f"words_cooccur: word_off must hold R + 1 >= 2 prefix sums, got {list(word_off.shape)}")
    _prefix(who, "ref_off", ref_off, R)
    _prefix(who, "cent_off", cent_off, R)
    _args.tensor(who, "co_off", co_off, "int64", (R + 1,))
    max_ref, max_hyp, co_total = int(max_ref), int(max_hyp), int(co_total)
    if co_total < 0:
        raise ValueError(f"words_cooccur: co_total={co_total} (the cells of every recording's table, >= 0)")
    co = torch.empty((max(co_total, 1),), dtype=torch.int32, device=rows.device)
    tally = torch.empty((R, 3), dtype=torch.int64, device=rows.device)
    check(engine.lib.sdk_words_cooccur(engine.ctx, rows.data_ptr() if W else None, ref.data_ptr() if W else None, word_off.data_ptr(), ref_off.data_ptr(),
                                       cent_off.data_ptr(), co_off.data_ptr(), R, W, max_ref, max_hyp, co_total, co.data_ptr(), tally.data_ptr(),
                                       _stream()), "sdk_words_cooccur")
    return co, tally


# ---- speaker samples (samples.py; csrc/samples.hip)
SAMPLES_SCAN_SPAN = 2048      # the packed frames one workgroup of sdk_samples_runs scans (SM_SPAN: 256 threads x 8 frames)


def samples_runs(engine, speakers: torch.Tensor, frame_off: torch.Tensor, cent_off: torch.Tensor, max_hyp: int, gap_frames: int, min_frames: int):
    """speakers [G, 2] int32 on the packed frame grid, frame_off, cent_off [R + 1] int32 prefix sums (diarize_ops.GroupTables), all on the
    device -> (run_off [R + 1] int32, rows [max(G // min_frames, 1), 4] int32) on the device: recording r's kept runs (speaker, g0, g1, solo) are
    rows[run_off[r]:run_off[r + 1]], the rows from run_off[R] on are not written (sdk_samples_runs; samples.py states the rule).  max_hyp:
    the largest K_r of the pack (at most words.MAX_WORD_SPEAKERS); gap_frames: the silent frames a run may bridge; min_frames: the solo
    frames a run must hold (at least 1).  Nothing waits.

    A function of the engine, not a method of it: Engine's public surface is pinned name for name (tests/test_ops_layout_cpu.py)."""
    who = "samples_runs"
    G = int(_args.tensor(who, "speakers", speakers, "int32", (None, 2)).shape[0])
    R = int(_args.tensor(who, "frame_off", frame_off, "int32", (None,)).shape[0]) - 1
    if R < 1:
        raise ValueError(f"samples_runs: frame_off must hold R + 1 >= 2 prefix sums, got {list(frame_off.shape)}")
    _prefix(who, "cent_off", cent_off, R)
    max_hyp, gap_frames, min_frames = int(max_hyp), int(gap_frames), int(min_frames)
    if max_hyp < 0 or max_hyp > 1024:
        raise ValueError(f"samples_runs: {max_hyp} hypothesis speakers in a recording (at most 1024)")
    if gap_frames < 0 or gap_frames >= 1 << 30:
        raise ValueError(f"samples_runs: gap_frames={gap_frames} (0 .. 2^30 - 1)")
    if min_frames < 1 or min_frames >= 1 << 30:
        raise ValueError(f"samples_runs: min_frames={min_frames} (1 .. 2^30 - 1)")
    if G >= 1 << 30:
        raise ValueError(f"samples_runs: G={G} frames in one pack (fewer than 2^30)")
    cap = G // min_frames
    run_off = torch.empty((R + 1,), dtype=torch.int32, device=speakers.device)
    rows = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=speakers.device)
    ws = engine._workspace("sdk_samples_runs_workspace_bytes", G)
    check(engine.lib.sdk_samples_runs(engine.ctx, speakers.data_ptr() if G else None, frame_off.data_ptr(), cent_off.data_ptr(), R, G, max_hyp, gap_frames,
                                      min_frames, run_off.data_ptr(), rows.data_ptr(), cap, ws.data_ptr(), ws.numel(), _stream()), "sdk_samples_runs")
    return run_off, rows


def samples_score(engine, E: torch.Tensor, clip_off: torch.Tensor, clip_spk: torch.Tensor, spk_off: torch.Tensor, n_speakers: int):
    """E [W, d] fp32 rows (read as they are; d a multiple of 64, at most diarize_host.MAX_ASSIGN_DIM), clip_off [M + 1] int32 (clip i holds the
    rows clip_off[i]:clip_off[i + 1]), clip_spk [M] int32 (the clip's speaker numbered over the pack: spk_off[r] + k), spk_off [R + 1] int32
    prefix sums of the recordings' speakers with spk_off[R] == n_speakers, all on the device -> (mean [S, d] float64, out_f [M, 2] float64 =
    (own, rival), out_i [M, 3] int32 = (rival_speaker local, windows, alone)) on the device (sdk_samples_score; samples.py states the rule).
    Nothing waits and E never goes to the host.

    A function of the engine, not a method of it: Engine's public surface is pinned name for name (tests/test_ops_layout_cpu.py)."""
    who = "samples_score"
    _args.tensor(who, "E", E, "float32", (None, None))
    W, d = int(E.shape[0]), _args.row_width(who, int(E.shape[1]))
    M = int(_args.tensor(who, "clip_off", clip_off, "int32", (None,)).shape[0]) - 1
    if M < 0:
        raise ValueError(f"samples_score: clip_off must hold M + 1 >= 1 prefix sums, got {list(clip_off.shape)}")
    _args.tensor(who, "clip_spk", clip_spk, "int32", (M,))
    R = int(_args.tensor(who, "spk_off", spk_off, "int32", (None,)).shape[0]) - 1
    if R < 1:
        raise ValueError(f"samples_score: spk_off must hold R + 1 >= 2 prefix sums, got {list(spk_off.shape)}")
    S = int(n_speakers)
    if S < 0 or S >= 1 << 24 or M >= 1 << 24 or W >= 1 << 24:
        raise ValueError(f"samples_score: W={W} windows, M={M} clips, S={S} speakers (fewer than 2^24 each)")
    dev = E.device
    mean = torch.empty((S, d), dtype=torch.float64, device=dev)
    out_f = torch.empty((M, 2), dtype=torch.float64, device=dev)
    out_i = torch.empty((M, 3), dtype=torch.int32, device=dev)
    ws = engine._workspace("sdk_samples_score_workspace_bytes", M, S, d)
    check(engine.lib.sdk_samples_score(engine.ctx, E.data_ptr() if W else None, W, d, clip_off.data_ptr(), clip_spk.data_ptr() if M else None, M,
                                       spk_off.data_ptr(), R, S, mean.data_ptr() if S else None, out_f.data_ptr() if M else None,
                                       out_i.data_ptr() if M else None, ws.data_ptr(), ws.numel(), _stream()), "sdk_samples_score")
    return mean, out_f, out_i
