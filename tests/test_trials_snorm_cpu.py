"""CPU checks of the AS-norm verification trials (trials_snorm.py, ops_score.trial_hist_snorm's argument refusals and the two backend entry
points' refusals): the numpy restatement is trials.counts_from_scores on the z the rule states, that z is snorm.py's z up to the
reciprocal (`* inv` against `/ std`), every argument that does not hold together is refused before any launch, and the refusals that the
older entry points pin stay."""
from __future__ import annotations

import subprocess
import sys

import numpy as np
import pytest
import torch
from conftest import PKG, ROOT, sub

T = sub("trials")
TS = sub("trials_snorm")
SN = sub("snorm")
OPS = sub("ops_score")
BK = sub("backend")

RULE_VARIABLES = ("SDK_COHORT", "SDK_COHORT_TOPK", "SDK_COHORT_THRESHOLD", "SDK_NO_TORCH", "SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA",
                  "SDK_SCORE_PLDA_DIM", "SDK_SCORE_PLDA_THRESHOLD", "SDK_SCORE_PLDA_COUNT", "SDK_SCORE_CALIBRATION")


def same(p, w):
    return (np.array_equal(p.hist, w.hist) and np.array_equal(p.under, w.under) and np.array_equal(p.over, w.over)
            and np.array_equal(p.nan, w.nan) and p.excluded == w.excluded)


def unit(X):
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def test_module_imports_neither_torch_nor_the_library():
    code = (f"import importlib, sys; importlib.import_module('{PKG}.trials_snorm'); "
            f"assert 'torch' not in sys.modules and '{PKG}._lib' not in sys.modules and '{PKG}.ops_score' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(ROOT))
    assert TS.SNORM_RANGE == (-64.0, 64.0) and 128.0 / 2 ** 24 < 7.7e-6


def test_host_restatement_is_counts_from_scores_on_the_stated_z():
    rng = np.random.default_rng(3)
    N, M, K = 37, 29, 32
    A, B = rng.standard_normal((N, K)), rng.standard_normal((M, K))
    ma, mb = rng.uniform(-8, 8, N), rng.uniform(-8, 8, M)
    ia, ib = rng.uniform(0.25, 4, N), rng.uniform(0.25, 4, M)
    ma[3], ib[5] = np.nan, np.inf                                    # a NaN row, a column of +-inf
    la, lb = rng.integers(-1, 4, N), rng.integers(-1, 4, M)
    sa, sb = rng.integers(-1, 3, N), rng.integers(-1, 3, M)
    S = A @ B.T
    Z = np.empty((N, M))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(N):                                           # the six operations, one at a time
            for j in range(M):
                da = np.float64(S[i, j]) - np.float64(ma[i])
                za = da * np.float64(ia[i])
                db = np.float64(S[i, j]) - np.float64(mb[j])
                zb = db * np.float64(ib[j])
                Z[i, j] = (za + zb) * np.float64(0.5)
    assert np.array_equal(TS.snorm_scores_host(A, B, ma, ia, mb, ib), Z, equal_nan=True)
    cls = T.trial_classes(la, sa, lb, sb)
    for lo, hi, shift, base in ((-64.0, 64.0, 12, 0), (-64.0, 64.0, 0, 4096 * 2048), (-4.0, 4.0, 12, 0), (-64.0, 64.0, 24, 1)):
        got = TS.trial_hist_snorm_host(A, B, ma, ia, mb, ib, la, sa, lb, sb, lo, hi, shift, base)
        assert same(got, T.counts_from_scores(Z, cls, lo, hi, shift, base))
        assert got.total() + int(got.nan.sum()) + got.excluded == N * M
    full = TS.trial_hist_snorm_host(A, B, ma, ia, mb, ib, la, sa, lb, sb, *TS.SNORM_RANGE)
    live3 = int((cls[3] >= 0).sum())
    assert int(full.nan.sum()) >= live3 > 0 and full.over.sum() + full.under.sum() >= int((cls[np.arange(N) != 3, 5] >= 0).sum()) > 0


def test_z_is_snorm_pys_z_up_to_the_reciprocal():
    rng = np.random.default_rng(4)
    d, nspk = 192, 9
    centres = rng.standard_normal((nspk, d))
    E = unit(centres[rng.integers(0, nspk, 120)] + 1.5 * rng.standard_normal((120, d)))
    P = unit(centres + 0.5 * rng.standard_normal((nspk, d)))
    C = unit(rng.standard_normal((400, d)))
    me, se = SN.cohort_stats_host(E, C, 50)
    mp, sp = SN.cohort_stats_host(P, C, 50)
    Z = TS.snorm_scores_host(E.astype(np.float64), P.astype(np.float64), me, 1.0 / se, mp, 1.0 / sp)
    idx, z, raw = SN.snorm_topk_host(E, me, se, P, mp, sp, k=1)
    assert (idx[:, 0] >= 0).all() and np.array_equal(idx[:, 0], np.argmax(Z, axis=1))
    win = Z[np.arange(len(E)), idx[:, 0]]
    assert np.abs(win - z[:, 0]).max() <= 1e-12 and np.abs(win).max() > 1.0
    with np.errstate(invalid="ignore"):
        whole = 0.5 * ((E.astype(np.float64) @ P.astype(np.float64).T - me[:, None]) / se[:, None]
                       + (E.astype(np.float64) @ P.astype(np.float64).T - mp[None, :]) / sp[None, :])
    assert np.abs(Z - whole).max() <= 1e-12


def test_host_restatement_refuses_what_does_not_belong_together():
    A, B = np.zeros((4, 16)), np.zeros((3, 16))
    v4, v3, i4, i3 = np.zeros(4), np.zeros(3), np.zeros(4, int), np.zeros(3, int)
    ok = dict(A=A, B=B, mean_a=v4, inv_a=v4, mean_b=v3, inv_b=v3, la=i4, sa=i4 - 1, lb=i3, sb=i3 - 1, lo=-1.0, hi=1.0)
    assert TS.trial_hist_snorm_host(**ok).total() == 12               # session -1 on both sides: nothing is excluded
    for kw in (dict(B=np.zeros((3, 32))), dict(A=np.zeros(16)), dict(mean_a=v3), dict(inv_a=v3), dict(mean_b=v4), dict(inv_b=np.zeros((3, 1))),
               dict(la=i3), dict(sb=i4), dict(lo=1.0, hi=1.0), dict(hi=float("inf")), dict(lo=float("nan")), dict(shift=25), dict(base=-1),
               dict(base=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            TS.trial_hist_snorm_host(**{**ok, **kw})


def test_wrapper_refuses_every_bad_argument_before_any_launch():
    """Host tensors reach every refusal but the device's own (the last): no engine is needed."""
    f8 = lambda *s: torch.zeros(s, dtype=torch.float64)              # noqa: E731
    i4 = lambda n: torch.zeros(n, dtype=torch.int32)                 # noqa: E731
    ok = dict(A=f8(8, 32), B=f8(6, 32), mean_a=f8(8), inv_a=f8(8), mean_b=f8(6), inv_b=f8(6), la=i4(8), sa=i4(8), lb=i4(6), sb=i4(6), lo=-1.0, hi=1.0)

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            OPS.trial_hist_snorm(None, **{**ok, **kw})

    refused("finite lo < hi", lo=1.0, hi=1.0)
    refused("finite lo < hi", lo=2.0, hi=1.0)
    refused("finite lo < hi", hi=float("inf"))
    refused("finite lo < hi", lo=float("nan"))
    refused("not a finite number above 0", lo=-1e308, hi=1e308)
    refused(r"shift=25", shift=25)
    refused(r"shift=-1", shift=-1)
    refused(r"base=-1", base=-1)
    refused(r"base=16777217", base=(1 << 24) + 1)
    refused(r"max_blocks=-1", max_blocks=-1)
    refused("A must be a contiguous float64 device tensor", A=np.zeros((8, 32)))
    refused("A must be a contiguous float64 device tensor", A=f8(8, 32).float())
    refused("A must be a contiguous float64 device tensor", A=f8(8))
    refused("A must be a contiguous float64 device tensor .* with strides", A=f8(32, 8).t())
    refused("there is no CPU path")                                  # everything else holds: the device comes last
    for name in ("mean_a", "inv_a", "mean_b", "inv_b", "la", "sa", "lb", "sb"):
        assert name in OPS.trial_hist_snorm.__code__.co_varnames


def test_library_refuses_bad_scalars_before_it_reads_the_context():
    """sdk_trial_hist_snorm checks K, N, M, shift, base, max_blocks, lo and scale first, then the context: without a device every call is
    refused (status 2), and the message says by which rule."""
    lib = sub("_lib").load_library()

    def raw(K=32, N=8, M=8, lo=-1.0, scale=2.0 ** 23, shift=12, base=0, max_blocks=0):
        rc = lib.sdk_trial_hist_snorm(None, None, N, None, M, K, None, None, None, None, None, None, None, None, lo, scale, shift, base, max_blocks,
                                      None, None)
        return rc, lib.sdk_last_error().decode()

    assert raw() == (2, "sdk_trial_hist_snorm: null context")
    for kw, text in ((dict(K=24), "K=24 not supported"), (dict(K=528), "K=528 not supported"), (dict(K=0), "K=0 not supported"),
                     (dict(N=0), "N=0 test rows"), (dict(M=(1 << 20) + 1), "M=1048577 model rows"), (dict(shift=25), "shift=25"),
                     (dict(shift=-1), "shift=-1"), (dict(base=-1), "base=-1"), (dict(base=(1 << 24) + 1), "base=16777217"),
                     (dict(max_blocks=-1), "max_blocks=-1"), (dict(scale=0.0), "scale=0"), (dict(scale=-1.0), "scale=-1"),
                     (dict(scale=float("inf")), "scale=inf"), (dict(scale=float("nan")), "scale=nan"), (dict(lo=float("nan")), "lo=nan"),
                     (dict(lo=float("-inf")), "lo=-inf")):
        rc, msg = raw(**kw)
        assert rc == 2 and msg.startswith("sdk_trial_hist_snorm: ") and text in msg, (kw, msg)


def test_entry_points_refuse_a_missing_cohort(monkeypatch):
    for v in RULE_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("SDK_ECAPA_WEIGHTS", "unused.npz")             # only silences the synthetic-weights notice; nothing is loaded here
    with pytest.raises(ValueError, match="evaluate_snorm: no cohort"):
        TS.evaluate_snorm(None, None, [0], [0], None, [0], [0], None, 10)
    with pytest.raises(ValueError, match="evaluate_snorm: topk is None"):
        TS.evaluate_snorm(None, None, [0], [0], None, [0], [0], object(), None)
    be = BK.Backend()
    assert be.rule.kind == "cosine" and be.cohort() is None
    with pytest.raises(ValueError, match="score_verification_snorm: no cohort"):
        BK.score_verification_snorm(be, ["a.wav"], ["ann"], [])
    with pytest.raises(ValueError, match="tune_cohort_threshold: no cohort"):
        BK.tune_cohort_threshold(be, ["a.wav"], ["ann"], [])
    with pytest.raises(ValueError, match="not a readable .npy matrix"):
        BK.score_verification_snorm(be, ["a.wav"], ["ann"], [], cohort="no-such-cohort.npy")
    wrong = SN.Cohort(np.eye(64, dtype=np.float32))
    with pytest.raises(ValueError, match="rows of d=64"):
        BK.score_verification_snorm(be, ["a.wav"], ["ann"], [], cohort=wrong)
    with pytest.raises(ValueError, match="topk=0"):
        BK.score_verification_snorm(be, ["a.wav"], ["ann"], [], cohort=SN.Cohort(np.eye(be.embedding_dim, dtype=np.float32)), topk=0)
    assert be._engine is None                                         # every refusal came before any device work
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    with pytest.raises(ValueError, match="score_verification_snorm: needs the torch engine"):
        BK.score_verification_snorm(BK.Backend(), ["a.wav"], ["ann"], [], cohort=wrong)


def test_the_older_entry_points_still_refuse_as_norm(monkeypatch):
    for v in RULE_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("SDK_ECAPA_WEIGHTS", "unused.npz")
    monkeypatch.setenv("SDK_COHORT", "cohort.npy")
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "1.0")
    be = BK.Backend()
    with pytest.raises(ValueError, match="AS-norm trials are not built"):
        be.rule.refuse_trials()
    with pytest.raises(ValueError, match="AS-norm trials are not built.*tune_cohort_threshold"):
        be.score_verification(["a.wav"], ["ann"], [])
    with pytest.raises(ValueError, match="AS-norm trials are not built"):
        BK.calibrate_verification(be, ["a.wav"], ["ann"], [])
    with pytest.raises(ValueError, match="'cosine' or 'plda'"):
        T.evaluate_scores(None, *([None] * 7), "snorm")
    assert be._engine is None
