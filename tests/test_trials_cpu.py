"""The count-based metric functions of trials.py (eer_from_counts, min_dcf_from_counts, det_from_counts, trial_hist_host) against the independent
brute-force reference tests/trials_ref.py, which evaluates every integer threshold that occurs.  No GPU: the passes come from trials.py's
own numpy restatement (counts_from_scores / trial_hist_host), the same counters the device returns."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trials_ref as TR  # noqa: E402
from conftest import sub  # noqa: E402

T = sub("trials")
LO, HI = T.COSINE_RANGE
EXACT = 1 << 13          # more zooms than there are coarse bins: min_dcf_exact must come out true


def passes(S, cls, lo=LO, hi=HI):
    coarse = T.counts_from_scores(S, cls, lo, hi)
    return coarse, (lambda b: T.counts_from_scores(S, cls, lo, hi, 0, T.BINS * b))


def check_against_reference(S, cls, lo=LO, hi=HI, p=0.01, cm=1.0, cf=1.0):
    coarse, zoom = passes(S, cls, lo, hi)
    ref = TR.metrics(S, cls, lo, hi, p, cm, cf)
    res = T.result_from_passes(coarse, zoom, "cosine", lo, hi, p, cm, cf, max_refine=EXACT)
    assert (res.n_target, res.n_nontarget, res.n_nan, res.n_excluded) == (ref["T"], ref["Nn"], ref["n_nan"], ref["n_excluded"])
    assert res.n_target + res.n_nontarget == coarse.total()
    assert res.t_star == ref["t_star"] and res.eer == ref["eer"] and res.eer_threshold == ref["eer_threshold"]
    assert res.min_dcf_exact and res.min_dcf == ref["min_dcf"] == res.min_dcf_lower
    loose = T.min_dcf_from_counts(coarse, zoom, lo, hi, p, cm, cf, max_refine=0)
    assert loose["n_zooms"] == 0 and loose["min_dcf_lower"] <= ref["min_dcf"] <= loose["min_dcf"]
    pm, pf, th = res.det_pmiss, res.det_pfa, res.det_thresholds
    assert pm.shape == pf.shape == th.shape == (4097,) and (np.diff(pm) >= 0).all() and (np.diff(pf) <= 0).all() and (np.diff(th) > 0).all()
    q, nan = TR.quantise(S, lo, hi)
    live = (np.asarray(cls).ravel() >= 0) & ~nan.ravel()
    for b in (0, 1, 2047, 2048, 2049, 4095, 4096):
        assert pm[b] == ((q.ravel() < 4096 * b) & live & (np.asarray(cls).ravel() == 1)).sum() / ref["T"]
        assert pf[b] == ((q.ravel() >= 4096 * b) & live & (np.asarray(cls).ravel() == 0)).sum() / ref["Nn"]
    return res, ref


@pytest.mark.parametrize("seed,nt,nn,sep,p", [(0, 40, 400, 0.5, 0.01), (1, 300, 5000, 0.3, 0.05), (2, 7, 9, 0.1, 0.5), (3, 1000, 1000, 0.8, 0.001)])
def test_small_random_sets(seed, nt, nn, sep, p):
    rng = np.random.default_rng(seed)
    S = np.concatenate([rng.normal(sep, 0.15, nt), rng.normal(0.0, 0.15, nn)]).clip(-1, 1)
    cls = np.concatenate([np.ones(nt, int), np.zeros(nn, int)])
    res, _ = check_against_reference(S, cls, p=p, cm=1.0, cf=1.0 if seed != 1 else 10.0)
    assert 0.0 <= res.eer <= 1.0 and LO <= res.eer_threshold <= HI


def test_random_set_on_a_wide_range_with_scores_outside_it():
    rng = np.random.default_rng(5)
    S = np.concatenate([rng.normal(3.0, 4.0, 500), rng.normal(-3.0, 4.0, 3000)])
    cls = np.concatenate([np.ones(500, int), np.zeros(3000, int)])
    res, _ = check_against_reference(S, cls, lo=-8.0, hi=8.0)
    assert res.counts.under.sum() > 0 and res.counts.over.sum() > 0


def test_perfectly_separable_scores_have_eer_zero():
    rng = np.random.default_rng(6)
    S = np.concatenate([rng.uniform(0.6, 0.9, 50), rng.uniform(-0.2, 0.3, 700)])
    cls = np.concatenate([np.ones(50, int), np.zeros(700, int)])
    res, _ = check_against_reference(S, cls)
    assert res.eer == 0.0 and res.min_dcf == 0.0 and S[50:].max() < res.eer_threshold <= S[:50].min()


def test_identical_distributions():
    rng = np.random.default_rng(7)
    s = rng.normal(0.1, 0.2, 600).clip(-1, 1)
    res, _ = check_against_reference(np.concatenate([s, s]), np.concatenate([np.ones(600, int), np.zeros(600, int)]))
    assert abs(res.eer - 0.5) < 0.01


def test_all_scores_in_one_fine_bin():
    S = np.full(30, 0.25)
    cls = np.arange(30) % 3 == 0
    res, ref = check_against_reference(S, cls.astype(int))
    q = int(TR.quantise(S[:1], LO, HI)[0][0])
    assert res.t_star == q + 1 and res.eer == 0.5


def test_t_star_zero():
    # every target lies below the range: the condition holds at t = 0 already
    S = np.concatenate([np.full(10, -2.0), np.linspace(-2.0, 0.5, 40)])
    cls = np.concatenate([np.ones(10, int), np.zeros(40, int)])
    res, ref = check_against_reference(S, cls)
    pfa0 = (S[10:] >= LO).sum() / 40
    assert res.t_star == 0 and res.eer == (1.0 + pfa0) / 2 and res.eer_threshold == LO


def test_a_crossing_outside_the_range_is_refused():
    S = np.concatenate([np.full(10, 2.0), np.full(40, 1.5)])           # everything above hi: fa(2^24) = Nn, miss(2^24) = 0
    cls = np.concatenate([np.ones(10, int), np.zeros(40, int)])
    coarse, zoom = passes(S, cls)
    assert TR.metrics(S, cls, LO, HI)["eer"] is None
    with pytest.raises(ValueError, match="over.*wider"):
        T.eer_from_counts(coarse, zoom, LO, HI)
    with pytest.raises(ValueError, match="wider"):
        T.result_from_passes(coarse, zoom, "cosine", LO, HI)


@pytest.mark.parametrize("cls", [np.ones(20, int), np.zeros(20, int), np.full(20, -1)])
def test_a_missing_class_is_refused(cls):
    S = np.linspace(-0.5, 0.5, 20)
    coarse, zoom = passes(S, cls)
    for call in (lambda: T.eer_from_counts(coarse, zoom, LO, HI), lambda: T.min_dcf_from_counts(coarse, zoom, LO, HI),
                 lambda: T.det_from_counts(coarse, LO, HI), lambda: T.result_from_passes(coarse, zoom, "cosine", LO, HI)):
        with pytest.raises(ValueError, match="both classes"):
            call()


def test_nan_and_excluded_trials_are_left_out_of_the_totals():
    rng = np.random.default_rng(8)
    S = np.concatenate([rng.normal(0.5, 0.2, 100), rng.normal(0.0, 0.2, 900)]).clip(-1, 1)
    cls = np.concatenate([np.ones(100, int), np.zeros(900, int)])
    S[[3, 50, 200, 201, 999]] = np.nan
    cls[[7, 8, 500, 50]] = -1                                        # 50 is both: excluded wins
    res, ref = check_against_reference(S, cls)
    assert res.n_nan == 4 and res.n_excluded == 4 and res.n_target == 100 - 2 - 2 and res.n_nontarget == 900 - 1 - 3
    assert res.counts.nan.tolist() == [3, 1]
    plain, _ = check_against_reference(S[(cls >= 0) & ~np.isnan(S)], cls[(cls >= 0) & ~np.isnan(S)])
    assert (plain.eer, plain.min_dcf, plain.eer_threshold) == (res.eer, res.min_dcf, res.eer_threshold)


def test_infinite_scores_are_below_and_above():
    S = np.asarray([-np.inf, np.inf, 0.2, 0.1, -np.inf, np.inf, HI, LO])
    cls = np.asarray([1, 1, 1, 0, 0, 0, 0, 1])
    coarse, _ = passes(S, cls)
    assert coarse.under.tolist() == [1, 1] and coarse.over.tolist() == [2, 1]          # a score exactly at hi is above; exactly at lo is q = 0
    assert coarse.hist[1][0] == 1 and coarse.nan.sum() == 0 and coarse.total() == 8


def test_every_trial_is_counted_exactly_once_in_every_pass():
    rng = np.random.default_rng(9)
    A = np.round(rng.uniform(-2, 2, (37, 16)) * 64) / 64
    B = np.round(rng.uniform(-2, 2, (29, 16)) * 64) / 64
    r = np.round(rng.uniform(-2, 2, 29) * 64) / 64
    r[4] = np.nan
    la, lb = rng.integers(-1, 4, 37), rng.integers(-1, 4, 29)
    sa, sb = rng.integers(-1, 3, 37), rng.integers(-1, 3, 29)
    cls = TR.classes(la, sa, lb, sb)
    assert np.array_equal(cls, T.trial_classes(la, sa, lb, sb))
    for shift, base in ((12, 0), (0, 4096 * 2048), (12, 4096), (24, 0), (24, 1), (0, 1 << 24), (5, 1000)):
        p = T.trial_hist_host(A, B, r, la, sa, lb, sb, -64.0, 64.0, shift, base)
        assert p.total() + int(p.nan.sum()) + p.excluded == 37 * 29 and p.excluded == int((cls < 0).sum())
        q, nan = TR.quantise(A @ B.T + r, -64.0, 64.0)
        for c in (0, 1):
            live = (cls == c) & ~nan
            bins = (np.clip(q, 0, (1 << 24) - 1) >> shift) - base
            want_under = (live & ((q < 0) | ((q < (1 << 24)) & (bins < 0)))).sum()
            want_hist = np.bincount(bins[live & (q >= 0) & (q < (1 << 24)) & (bins >= 0) & (bins < 4096)], minlength=4096)
            assert p.under[c] == want_under and np.array_equal(p.hist[c], want_hist) and p.nan[c] == ((cls == c) & nan).sum()


def test_refused_ranges():
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (-np.inf, 1.0), (0.0, np.nan), (-1e308, 1e308)):
        with pytest.raises(ValueError):
            T.scale_of(lo, hi)


def test_the_module_imports_neither_torch_nor_the_library():
    import subprocess
    code = ("import importlib, sys; importlib.import_module('speaker-diarization-toolkit_amd.trials'); "
            "assert 'torch' not in sys.modules and 'speaker-diarization-toolkit_amd._lib' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
