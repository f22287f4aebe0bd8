"""GPU checks of the AS-norm trial histogram (sdk_trial_hist_snorm, ops_score.trial_hist_snorm), of trials_snorm.evaluate_snorm and of
backend.score_verification_snorm / backend.tune_cohort_threshold.

Bit-exact cases.  Entries of A and B that are multiples of 2^-6 of magnitude <= 2 (tests/test_trials_gpu.py): every product is a multiple of
2^-12 and every partial sum stays below 2^11, so s is exact in float64 in any order and the device's s equals numpy's bit for bit.  The six
operations of z and the two of t are single IEEE operations on both sides (the kernel's file is compiled without contraction), so all 8199
counters must equal trials_snorm.trial_hist_snorm_host - for any float64 means and reciprocals.

The sandwich for rounded inputs.  tests/test_trials_gpu.py bounds the device's product against the extended-precision product rounded once
to float64 (S): |s_dev - S| <= delta = (K + 3) u a, u = 2^-53, a(i, j) = sum_k |A_ik B_jk| (derived there for a chain of K roundings with r;
without r the chain has one rounding fewer, so the bound holds with room).  The exact z of S is Z = ((S - ma) ia + (S - mb) ib) / 2.  The
device forms z from s_dev = S + e, |e| <= delta, in five rounded operations and an exact halving:
    fl(s_dev - ma) = (s_dev - ma)(1 + e1),   fl(. * ia) = (.)(1 + e2)   and the same on the model side (e3, e4),   fl(za + zb) = (.)(1 + e5)
so with Ta = (|S - ma| + delta) ia and Tb = (|S - mb| + delta) ib, which bound the two halves before rounding,
    |z_dev - Z| <= delta (ia + ib) / 2 + ((1 + u)^3 - 1) (Ta + Tb) / 2 <= delta (ia + ib) / 2 + 2 u (Ta + Tb).
The host reference forms Z in extended precision from S (five operations of relative error 2^-64 each: below u (Ta + Tb) / 256) and rounds
it once to float64 (u |Z| <= u (Ta + Tb) / 2).  Together:
    |z_dev - Zref| <= dz = delta (ia + ib) / 2 + 3 u (Ta + Tb).
q is non-decreasing in z, so q(Zref - dz) <= q(device) <= q(Zref + dz) for every trial; the cumulative counts and t* are sandwiched as in
tests/test_trials_gpu.py.  The statistics are the device's own (Engine.cohort_stats, widened, inverted): both sides read the same numbers.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trials_ref as TR  # noqa: E402
from conftest import ROOT, sub  # noqa: E402

pytestmark = pytest.mark.gpu

T = sub("trials")
TS = sub("trials_snorm")
OPS = sub("ops_score")
U53 = 2.0 ** -53
LD = np.longdouble
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the sandwich's host reference needs an extended-precision long double"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_hist(engine, A, B, ma, ia, mb, ib, la, sa, lb, sb, lo, hi, shift=12, base=0, max_blocks=0):
    out = OPS.trial_hist_snorm(engine, dev(A), dev(B), dev(ma), dev(ia), dev(mb), dev(ib), dev(la.astype(np.int32)), dev(sa.astype(np.int32)),
                               dev(lb.astype(np.int32)), dev(sb.astype(np.int32)), lo, hi, shift=shift, base=base, max_blocks=max_blocks)
    torch.cuda.synchronize()
    return T.counts_to_host(out)


def same(p, w):
    return (np.array_equal(p.hist, w.hist) and np.array_equal(p.under, w.under) and np.array_equal(p.over, w.over)
            and np.array_equal(p.nan, w.nan) and p.excluded == w.excluded)


def grid_inputs(N, M, K, seed):
    """A, B on the 2^-6 grid, labels and sessions as grid_inputs of tests/test_trials_gpu.py; float64 means in [-8, 8], reciprocals in [0.25, 4]."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-128, 129, (N, K)) / 64.0
    B = rng.integers(-128, 129, (M, K)) / 64.0
    ma, mb = rng.uniform(-8.0, 8.0, N), rng.uniform(-8.0, 8.0, M)
    ia, ib = rng.uniform(0.25, 4.0, N), rng.uniform(0.25, 4.0, M)
    la, lb = rng.integers(-1, 5, N), rng.integers(-1, 5, M)
    sa, sb = rng.integers(-1, 4, N), rng.integers(-1, 4, M)
    return A, B, ma, ia, mb, ib, la, sa, lb, sb


# ---- bit-exact histograms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,K,max_blocks", [(1, 1, 16, 0), (63, 65, 16, 0), (64, 64, 192, 0), (130, 200, 256, 0), (130, 200, 256, 1)])
def test_histograms_are_bit_exact_on_exact_products(engine, N, M, K, max_blocks):
    x = list(grid_inputs(N, M, K, 100 + N + K))
    if N == 1:
        x[6][:], x[8][:], x[7][:], x[9][:] = 2, 2, 0, 1
    lo, hi = -512.0, 512.0
    want = TS.trial_hist_snorm_host(*x, lo, hi)
    assert int(want.hist.sum()) >= 0.99 * want.total() > 0          # the reference itself bins its trials: the comparison is not one of under / over
    got = gpu_hist(engine, *x, lo, hi, max_blocks=max_blocks)
    assert got.total() + int(got.nan.sum()) + got.excluded == N * M
    assert same(got, want)
    b = int(np.argmax(want.hist.sum(axis=0)))
    wantz = TS.trial_hist_snorm_host(*x, lo, hi, 0, 4096 * b)
    gotz = gpu_hist(engine, *x, lo, hi, 0, 4096 * b, max_blocks=max_blocks)
    assert gotz.total() == got.total() and int(gotz.hist.sum()) == int(want.hist[:, b].sum()) > 0
    assert same(gotz, wantz)


# ---- the three trial kernels share one tile walk: with neutral statistics they must count the same trials ------------------------------------
@pytest.mark.parametrize("max_blocks", [0, 1])
@pytest.mark.parametrize("N,M,K", [(63, 65, 16), (130, 200, 256)])
def test_neutral_statistics_equal_the_plain_histogram_and_the_calibration_counts(engine, N, M, K, max_blocks):
    """mean = 0 and inv = 1 on both sides: z = (s + s) * 0.5 = s exactly, so trial_hist_snorm returns Engine.trial_hist's 8199 counters at
    r = 0 on the same rows, labels and sessions, at the coarse pass and at a zoom pass; trial_calib's n + nonfinite and excluded are the
    class totals and excluded of that pass.  Integer equality throughout."""
    A, B, _, _, _, _, la, sa, lb, sb = grid_inputs(N, M, K, 300 + N + K)
    assert (la < 0).any() and (lb < 0).any() and ((sa[:, None] >= 0) & (sa[:, None] == sb[None, :])).any()
    la32, sa32, lb32, sb32 = (dev(v.astype(np.int32)) for v in (la, sa, lb, sb))
    dA, dB, zeros_m = dev(A), dev(B), dev(np.zeros(M))
    lo, hi = -512.0, 512.0

    def plain(shift, base):
        out = engine.trial_hist(dA, dB, zeros_m, la32, sa32, lb32, sb32, lo, hi, shift=shift, base=base, max_blocks=max_blocks)
        torch.cuda.synchronize()
        return T.counts_to_host(out)

    def snorm(shift, base):
        return gpu_hist(engine, A, B, np.zeros(N), np.ones(N), np.zeros(M), np.ones(M), la, sa, lb, sb, lo, hi, shift, base, max_blocks)

    coarse = plain(12, 0)
    assert coarse.excluded > 0 and int(coarse.hist[0].sum()) > 0 and int(coarse.hist[1].sum()) > 0
    assert coarse.total() + int(coarse.nan.sum()) + coarse.excluded == N * M
    assert same(snorm(12, 0), coarse)
    b = int(np.argmax(coarse.hist.sum(axis=0)))
    zoom = plain(0, 4096 * b)
    assert int(zoom.hist.sum()) == int(coarse.hist[:, b].sum()) > 0
    assert same(snorm(0, 4096 * b), zoom)
    n, _, nonfinite, excluded = OPS.trial_calib(engine, dA, dB, zeros_m, la32, sa32, lb32, sb32, 1.0, 0.0, max_blocks=max_blocks)
    torch.cuda.synchronize()
    per_class = coarse.hist.sum(axis=1) + coarse.under + coarse.over + coarse.nan
    assert np.array_equal(n.cpu().numpy() + nonfinite.cpu().numpy(), per_class)
    assert int(excluded.item()) == coarse.excluded


# ---- special values --------------------------------------------------------------------------------------------------------------------------
def test_special_statistics_exclusions_and_empty_ranges(engine):
    K = 16
    A = np.zeros((5, K))
    A[:, 0] = [1.0, 0.5, 0.25, -1.0, 2.0]
    B = np.zeros((6, K))
    B[:, 0] = 1.0                                                    # s(i, j) = A[i, 0]
    ma, ia = np.asarray([0.0, np.nan, 0.25, 0.0, 0.0]), np.asarray([1.0, 1.0, np.inf, np.inf, 1.0])
    mb, ib = np.asarray([0.0, 0.0, 0.0, 0.0, 0.0, 0.5]), np.asarray([1.0, 1.0, 1.0, 1.0, 1.0, np.inf])
    la, sa = np.asarray([0, 1, 0, 2, 0]), np.full(5, -1)
    lb, sb = np.asarray([0, 1, 0, 2, 1, 0]), np.full(6, -1)
    x = (A, B, ma, ia, mb, ib, la, sa, lb, sb)
    lo, hi = TS.SNORM_RANGE
    got = gpu_hist(engine, *x, lo, hi)
    assert same(got, TS.trial_hist_snorm_host(*x, lo, hi))
    # by hand: row 1 has a NaN mean (6 NaN); row 2 has inv = +inf and s == mean: 0 * inf = NaN (6 more); row 3 has inv = +inf and s < mean:
    # -inf, under (6); column 5 has inv = +inf and s > mean in rows 0 and 4: +inf, over (2); rows 0 and 4 against columns 0 .. 4: z = s (10)
    assert got.excluded == 0 and int(got.nan.sum()) == 12 and int(got.under.sum()) == 6 and int(got.over.sum()) == 2 and int(got.hist.sum()) == 10
    assert got.nan.tolist() == [7, 5] and got.under.tolist() == [5, 1] and got.over.tolist() == [0, 2]
    assert got.total() + int(got.nan.sum()) + got.excluded == 30
    # every trial excluded: by label, and by one shared session
    none = gpu_hist(engine, A, B, ma, ia, mb, ib, np.full(5, -1), sa, lb, sb, lo, hi)
    assert none.excluded == 30 and none.total() == 0 and none.nan.sum() == 0
    one_session = gpu_hist(engine, A, B, ma, ia, mb, ib, la, np.zeros(5, int), lb, np.zeros(6, int), lo, hi)
    assert one_session.excluded == 30 and one_session.total() == 0 and one_session.nan.sum() == 0
    # bases that leave nothing in range: the finite trials go under (or over), the NaN stay NaN
    for shift, base in ((12, 4096), (0, 1 << 24), (24, 1), (24, 0)):
        g = gpu_hist(engine, *x, lo, hi, shift, base)
        assert same(g, TS.trial_hist_snorm_host(*x, lo, hi, shift, base))
        assert g.total() + int(g.nan.sum()) + g.excluded == 30 and int(g.nan.sum()) == 12
        if base:
            assert g.hist.sum() == 0 and int(g.under.sum()) == 16 and int(g.over.sum()) == 2
    tiny = gpu_hist(engine, *x, 1000.0, 1001.0)                       # every finite z lies below the range
    assert tiny.hist.sum() == 0 and int(tiny.under.sum()) == 16 and int(tiny.over.sum()) == 2 and int(tiny.nan.sum()) == 12


# ---- rounded inputs: the sandwich --------------------------------------------------------------------------------------------------------
def unit(X):
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def device_statistics(engine, E32, C32, topk):
    """The device's own statistics of fp32 rows (Engine.cohort_stats, widened, inverted) on the host: (mean, inv) float64."""
    mean, inv = TS.cohort_statistics(engine, dev(E32), dev(C32), topk)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), inv.cpu().numpy()


def reference_and_dz(A, B, ma, ia, mb, ib):
    """(Zref: z in extended precision from the extended-precision product rounded once to float64, itself rounded once; dz) - the module
    docstring's bound."""
    K = A.shape[1]
    S = (A.astype(LD) @ B.T.astype(LD)).astype(np.float64)
    delta = (K + 3) * U53 * (np.abs(A) @ np.abs(B).T)
    Sl = S.astype(LD)
    Z = (((Sl - ma.astype(LD)[:, None]) * ia.astype(LD)[:, None] + (Sl - mb.astype(LD)[None, :]) * ib.astype(LD)[None, :]) * LD(0.5)).astype(np.float64)
    Ta, Tb = (np.abs(S - ma[:, None]) + delta) * ia[:, None], (np.abs(S - mb[None, :]) + delta) * ib[None, :]
    dz = (delta * (ia[:, None] + ib[None, :]) / 2 + 3 * U53 * (Ta + Tb)) * (1 + 2.0 ** -40)
    return Z, dz


def test_unit_rows_with_real_statistics_inside_the_sandwich(engine):
    rng = np.random.default_rng(11)
    N, M, K, nspk = 150, 170, 192, 6
    centres = rng.standard_normal((nspk, K))
    la, lb = rng.integers(0, nspk, N), rng.integers(0, nspk, M)
    E, P = unit(centres[la] + 1.5 * rng.standard_normal((N, K))), unit(centres[lb] + 1.5 * rng.standard_normal((M, K)))
    C = unit(rng.standard_normal((400, K)))
    sa, sb = rng.integers(-1, 5, N), rng.integers(-1, 5, M)
    ma, ia = device_statistics(engine, E, C, 50)
    mb, ib = device_statistics(engine, P, C, 50)
    assert np.isfinite(ma).all() and np.isfinite(mb).all() and (ia > 0).all() and (ib > 0).all() and max(ia.max(), ib.max()) <= 1e6 * (1 + 1e-6)
    A, B = E.astype(np.float64), P.astype(np.float64)
    lo, hi = TS.SNORM_RANGE
    Z, dz = reference_and_dz(A, B, ma, ia, mb, ib)
    cls = TR.classes(la, sa, lb, sb)
    x = (A, B, ma, ia, mb, ib, la, sa, lb, sb)
    got = gpu_hist(engine, *x, lo, hi)
    q_ref, nan_ref = TR.quantise(Z, lo, hi)
    live_all = (cls >= 0) & ~nan_ref
    outside = int(((q_ref < 0) | (q_ref >= TR.QMAX))[live_all].sum())
    assert not nan_ref.any() and outside < 0.01 * int(live_all.sum())
    q_hi, nan = TR.quantise(Z + dz, lo, hi)
    q_lo, _ = TR.quantise(Z - dz, lo, hi)
    edges = 4096 * np.arange(4097)
    for c in (0, 1):
        live = (cls == c) & ~nan
        cum = int(got.under[c]) + np.concatenate([[0], np.cumsum(got.hist[c])])
        at_least = np.searchsorted(np.sort(q_hi[live]), edges, side="left")       # trials certainly below the edge
        at_most = np.searchsorted(np.sort(q_lo[live]), edges, side="left")
        assert (at_least <= cum).all() and (cum <= at_most).all()
        assert int(got.nan[c]) == 0
        assert cum[-1] + int(got.over[c]) == int(live.sum())
    res = T.result_from_passes(got, lambda b: gpu_hist(engine, *x, lo, hi, 0, 4096 * b), "snorm", lo, hi)
    t_lo, t_hi = TR.metrics(Z - dz, cls, lo, hi)["t_star"], TR.metrics(Z + dz, cls, lo, hi)["t_star"]
    assert t_lo <= res.t_star <= t_hi
    scale = T.scale_of(lo, hi)
    assert lo + t_lo / scale <= res.eer_threshold <= lo + t_hi / scale
    print(f"snorm sandwich K={K}: worst dz {float(dz.max()):.3e}, |z| up to {float(np.abs(Z).max()):.2f}, inv up to {float(max(ia.max(), ib.max())):.1f}, "
          f"{outside} outside the range, t* in [{t_lo}, {t_hi}] -> {res.t_star}, eer {res.eer:.4f} at {res.eer_threshold:.4f}")


# ---- trials_snorm.evaluate_snorm end to end -------------------------------------------------------------------------------------------------
def generated(seed=21, N=300, P=200, d=192, nspk=10):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((nspk, d))
    la, lb = np.arange(N) % nspk, np.arange(P) % nspk
    return (unit(centres[la] + 2.0 * rng.standard_normal((N, d))), la, np.arange(N) % 7,
            unit(centres[lb] + 2.0 * rng.standard_normal((P, d))), lb, np.where(np.arange(P) % 3 == 0, -1, np.arange(P) % 7),
            unit(rng.standard_normal((400, d))))


def test_evaluate_snorm_equals_the_brute_force(engine):
    Et, la, sa, Em, lb, sb, C = generated()
    topk = 50
    res = TS.evaluate_snorm(engine, dev(Et), la, sa, dev(Em), lb, sb, dev(C), topk, max_refine=4096)
    ma, ia = device_statistics(engine, Et, C, topk)
    mb, ib = device_statistics(engine, Em, C, topk)
    Z, dz = reference_and_dz(Et.astype(np.float64), Em.astype(np.float64), ma, ia, mb, ib)
    cls = TR.classes(la, sa, lb, sb)
    lo, hi = TS.SNORM_RANGE
    # no scored trial lies within dz of a cell edge of the q scale (a fact of the seeded inputs): q(device) = q(Zref) for every trial, and
    # the device's metrics must EQUAL the brute force on Zref
    q_lo, nan = TR.quantise(Z - dz, lo, hi)
    q_hi, _ = TR.quantise(Z + dz, lo, hi)
    live = (cls >= 0) & ~nan
    assert not nan.any() and np.array_equal(q_lo[live], q_hi[live])
    ref = TR.metrics(Z, cls, lo, hi)
    assert (res.n_target, res.n_nontarget, res.n_nan, res.n_excluded) == (ref["T"], ref["Nn"], 0, ref["n_excluded"])
    assert res.n_excluded > 0 and res.n_target + res.n_nontarget + res.n_excluded == 300 * 200 and (res.test_rows, res.model_rows) == (300, 200)
    assert res.t_star == ref["t_star"] and res.eer == ref["eer"] and res.eer_threshold == ref["eer_threshold"]
    assert res.min_dcf == ref["min_dcf"] and res.min_dcf_exact
    assert res.kind == "snorm" and res.score_range == TS.SNORM_RANGE and 0.0 < res.eer < 0.5
    q, _ = TR.quantise(Z, lo, hi)
    edges = 4096 * np.arange(4097)
    for c, rate in ((1, res.det_pmiss), (0, res.det_pfa)):           # the DET counts at the 4097 coarse thresholds
        qs = np.sort(q[(cls == c) & ~nan])
        below = np.searchsorted(qs, edges, side="left")
        cum = int(res.counts.under[c]) + np.concatenate([[0], np.cumsum(res.counts.hist[c])])
        assert np.array_equal(cum, below)
        count = below if c == 1 else len(qs) - below
        assert np.array_equal(rate, np.asarray([int(v) / len(qs) for v in count]))
    assert np.array_equal(res.det_thresholds, np.asarray([lo + (4096 * b) / T.scale_of(lo, hi) for b in range(4097)]))
    print(f"evaluate snorm: eer {res.eer:.4f} at z = {res.eer_threshold:.4f}, min_dcf {res.min_dcf:.4f} at {res.min_dcf_threshold:.4f}, "
          f"{res.n_zooms} zooms, |z| up to {float(np.abs(Z).max()):.2f}")


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_identical_counters(engine):
    A, B, ma, ia, mb, ib, la, sa, lb, sb = grid_inputs(300, 260, 64, 7)
    A, B = A + 1e-3 * np.random.default_rng(1).standard_normal(A.shape), B * (1 + 2.0 ** -30)       # rounded inputs
    runs = [gpu_hist(engine, A, B, ma, ia, mb, ib, la, sa, lb, sb, -256.0, 256.0, max_blocks=mb_) for mb_ in (0, 0, 3)]
    assert same(runs[0], runs[1]) and same(runs[0], runs[2]) and int(runs[0].hist.sum()) > 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    x = grid_inputs(8, 8, 32, 6)
    d = [dev(v) for v in x[:6]] + [dev(v.astype(np.int32)) for v in x[6:]]
    out = torch.zeros(8199, dtype=torch.int64, device="cuda")
    lib, ctx = engine.lib, engine.ctx
    NULL = object()

    def raw(K=32, N=8, M=8, lo=-1.0, scale=2.0 ** 23, shift=12, base=0, max_blocks=0, null=None, A_=None):
        p = [None if null == i else t.data_ptr() for i, t in enumerate(d)]
        if A_ is not None:
            p[0] = None if A_ is NULL else A_
        return lib.sdk_trial_hist_snorm(ctx, p[0], N, p[1], M, K, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], lo, scale, shift, base, max_blocks,
                                        None if null == 10 else out.data_ptr(), None)

    assert raw() == 0
    for kw in (dict(K=24), dict(K=528), dict(K=0), dict(shift=25), dict(shift=-1), dict(base=-1), dict(base=(1 << 24) + 1), dict(N=0),
               dict(M=(1 << 20) + 1), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=0.0), dict(scale=-1.0),      # lo >= hi
               dict(lo=float("nan")), dict(lo=float("-inf")), dict(max_blocks=-1), dict(A_=NULL), dict(A_=d[0].data_ptr() + 8),
               *(dict(null=i) for i in range(11))):
        assert raw(**kw) == 2, kw
        assert b"sdk_trial_hist_snorm" in lib.sdk_last_error()
    torch.cuda.synchronize()

    def call(lo=-1.0, hi=1.0, **kw):
        names = ("A", "B", "mean_a", "inv_a", "mean_b", "inv_b", "la", "sa", "lb", "sb")
        a = {**dict(zip(names, d)), **{k: v for k, v in kw.items() if k in names}}
        return OPS.trial_hist_snorm(engine, *(a[n] for n in names), lo, hi, **{k: v for k, v in kw.items() if k not in names})

    assert int(call()[0].sum()) >= 0
    wide = torch.zeros((8, 528), dtype=torch.float64, device="cuda")
    odd = torch.zeros((8, 24), dtype=torch.float64, device="cuda")
    big = torch.zeros(9, dtype=torch.float64, device="cuda")
    for bad in (dict(A=odd, B=odd), dict(A=wide, B=wide), dict(shift=25), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(lo=-1e308, hi=1e308),
                dict(hi=float("inf")), dict(lo=float("nan")), dict(base=-1), dict(max_blocks=-1), dict(A=d[0].float()), dict(A=d[0].cpu()),
                dict(B=torch.zeros((8, 16), dtype=torch.float64, device="cuda")), dict(mean_a=big), dict(inv_a=d[3].float()), dict(mean_b=big),
                dict(inv_b=d[5].cpu()), dict(la=d[6].long()), dict(sb=torch.zeros(9, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            call(**bad)


# ---- the Backend ---------------------------------------------------------------------------------------------------------------------------
def test_backend_tune_cohort_threshold(tmp_path, monkeypatch):
    sys.path.insert(0, str(ROOT / "evals"))
    from run_eval import render_voice
    wav, BK = sub("wav"), sub("backend")
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    for v in ("SDK_COHORT", "SDK_COHORT_THRESHOLD", "SDK_COHORT_TOPK", "SDK_NO_TORCH", "SDK_SCORE_PLDA_DIM", "SDK_SCORE_PLDA_THRESHOLD",
              "SDK_SCORE_PLDA_COUNT", "SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA", "SDK_SCORE_CALIBRATION"):
        monkeypatch.delenv(v, raising=False)
    be = BK.Backend()

    def recording(name, tag, seconds, seed):
        path = tmp_path / f"{name}.wav"
        wav.write_wav_s16(path, render_voice(tag, seconds, seed))
        return path

    profiles = []
    for i, (sid, takes) in enumerate((("ann", 2), ("bob", 1), ("cy", 1))):
        embs = []
        for t in range(takes):
            rec = be.enroll_speaker(recording(f"enroll_{sid}_{t}", sid, 5.0, 100 + 7 * i + 50 * t))
            embs.append({"id": f"emb-{sid}-{t}", "external_id": rec["external_id"], "model_version": rec["model_version"], "trust_level": "high"})
        profiles.append({"id": sid, "names": {"default": sid.title()}, "embeddings": {"mi355x": embs}})
    paths = [recording(f"dev_{j}", tag, 4.0, 300 + j) for j, tag in enumerate(("ann", "bob", "cy", "stranger"))]
    ids = ["ann", "bob", "cy", "nobody-enrolled"]
    cohort_path = tmp_path / "cohort.npy"
    made = be.make_cohort([recording(f"imp_{j}", f"impostor-{j}", 3.0, 500 + j) for j in range(8)], cohort_path)
    assert made["n_recordings"] == 8

    with pytest.raises(ValueError, match="no cohort"):
        BK.tune_cohort_threshold(be, paths, ids, profiles)
    out = BK.tune_cohort_threshold(be, paths, ids, profiles, cohort=cohort_path)
    assert {"kind", "eer", "eer_threshold", "min_dcf", "min_dcf_threshold", "min_dcf_lower", "min_dcf_exact", "n_target", "n_nontarget", "n_nan",
            "n_excluded", "n_test_rows", "n_model_rows", "score_range", "result", "cohort_digest", "topk"} == set(out)
    lo, hi = out["score_range"]
    print(f"tune_cohort_threshold: {out['n_test_rows']} windows x {out['n_model_rows']} model rows, topk {out['topk']}, eer {out['eer']:.4f} at "
          f"z = {out['eer_threshold']:.4f}, min_dcf {out['min_dcf']:.4f} at {out['min_dcf_threshold']:.4f}, under {out['result'].counts.under.tolist()}, "
          f"over {out['result'].counts.over.tolist()}")
    assert out["kind"] == "snorm" and (lo, hi) == TS.SNORM_RANGE and out["topk"] == 8
    assert out["cohort_digest"] == sub("snorm").Cohort.load(cohort_path, be.embedding_dim).digest
    cos = be.score_verification(paths, ids, profiles)
    assert cos.kind == "cosine"
    assert (out["n_target"], out["n_nontarget"], out["n_excluded"]) == (cos.n_target, cos.n_nontarget, cos.n_excluded)
    assert (out["n_test_rows"], out["n_model_rows"], out["n_nan"]) == (cos.test_rows, cos.model_rows, 0)
    assert np.isfinite(out["eer_threshold"]) and lo <= out["eer_threshold"] <= hi
    assert np.isfinite(out["min_dcf_threshold"]) and lo <= out["min_dcf_threshold"] <= hi
    assert 0.0 <= out["eer"] <= 1.0 and out["min_dcf_lower"] <= out["min_dcf"]
    res = BK.score_verification_snorm(be, paths, ids, profiles, cohort=sub("snorm").Cohort.load(cohort_path, be.embedding_dim))
    assert same(res.counts, out["result"].counts) and res.eer == out["eer"] and res.eer_threshold == out["eer_threshold"]

    # the tuned threshold is what SDK_COHORT_THRESHOLD takes: a backend configured with it identifies, and evaluates itself to the same result
    monkeypatch.setenv("SDK_COHORT", str(cohort_path))
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", repr(float(out["eer_threshold"])))
    be2 = BK.Backend()
    assert be2.rule.kind == "snorm" and be2.cohort_threshold == out["eer_threshold"]
    hits = be2.identify_speaker(paths[0], profiles)
    assert isinstance(hits, list) and all("norm_score" in h and h["norm_score"] >= out["eer_threshold"] for h in hits)
    res2 = BK.score_verification_snorm(be2, paths, ids, profiles)
    assert res2.kind == "snorm" and same(res2.counts, out["result"].counts)
    assert (res2.eer, res2.eer_threshold, res2.min_dcf, res2.min_dcf_threshold, res2.t_star) == (
        out["eer"], out["eer_threshold"], out["min_dcf"], out["min_dcf_threshold"], out["result"].t_star)
    with pytest.raises(ValueError, match="AS-norm trials are not built"):
        be2.score_verification(paths, ids, profiles)
