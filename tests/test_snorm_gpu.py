"""GPU checks of the adaptive score normalisation (sdk_cohort_stats, sdk_affinity_topk_snorm; Engine.cohort_stats, Engine.affinity_topk_snorm;
the Backend's normalised identify path) against the independent float64 reference tests/snorm_ref.py, which reads the same fp32 values.

The arithmetic bound.  An fp32 dot product of unit rows (one fused-multiply-add chain over d columns) errs by at most d 2^-24.  The mean of the
sorted top-K and their standard deviation are both 1-Lipschitz in the largest score error, so a selection that differs near a tie adds nothing;
a factor 2 covers the fp32 rounding of the outputs and the float64 accumulation: |mean - ref| and |std - ref| <= SCORE_BOUND(d) = 2 d 2^-24.
A normalised score z = ((s - m_e) / s_e + (s - m_p) / s_p) / 2 computed from EXACT statistics moves by at most |ds| / min(s_e, s_p); the
issue's element bound 4 SCORE_BOUND (1 + |z_ref|) / min(s_e, s_p) also covers z's own fp32 rounding.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partial_width as PW  # noqa: E402
import snorm_ref as SR  # noqa: E402
from conftest import ROOT, sub  # noqa: E402

pytestmark = pytest.mark.gpu

LIB = sub("_lib")
SN = sub("snorm")
STD_FLOOR32 = float(np.float32(SR.STD_FLOOR))


def score_bound(d):
    return 2.0 * d * 2.0 ** -24


def unit(x):
    x = np.asarray(x, dtype=np.float64)
    return np.ascontiguousarray((x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def block_rows(M):
    """Rows of one row block of sdk_cohort_stats for a cohort of M rows, read back from the workspace size: the least N at which it stops growing."""
    ws = LIB.load_library().sdk_cohort_stats_workspace_bytes
    cap = ws(1 << 30, M, 1)
    lo, hi = 1, 1 << 30
    while lo < hi:
        mid = (lo + hi) // 2
        if ws(mid, M, 1) >= cap:
            hi = mid
        else:
            lo = mid + 1
    return lo


def gpu_stats(engine, E, Cn, K):
    mean, std = engine.cohort_stats(dev(E), dev(Cn), K)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), std.cpu().numpy()


# ---- 1. statistics against float64 ---------------------------------------------------------------------------------------------------
# the last two: the widths at which the second column of a thread (tid + 256) is live for wave 0 only (320) and for every wave but the last (448).
# Checked on the CPU (tests/test_snorm_cpu.py prints it): without the columns 256.. the reference's statistics move by 253 and 537 x the bound
STAT_CASES = [(1, 64, 1, 64), (33, 257, 100, 192), (70, 1000, 300, 192), (5, 4099, 4099, 192), (5, 4099, 4098, 192), (3, 300, 7, 512),
              (33, 257, 100, 320), (3, 300, 7, 448)]
_worst = {}


def stats_rows(N, M, d, seed):
    rng = np.random.default_rng(seed)
    return unit(rng.standard_normal((N, d))), unit(rng.standard_normal((M, d)))


def check_stats(engine, N, M, K, d, seed):
    E, Cn = stats_rows(N, M, d, seed)
    rmean, rstd = SR.cohort_stats(E, Cn, K)
    b = score_bound(d)
    if d in PW.WIDTHS:                                                 # on the reference alone, before the device is asked
        SR.second_column_weight_stats(f"cohort_stats N={N} M={M} K={K} d={d}", E, Cn, K, (rmean, rstd), b)
    mean, std = gpu_stats(engine, E, Cn, K)
    em, es = float(np.abs(mean - rmean).max()), float(np.abs(std - rstd).max())
    _worst[(N, M, K, d)] = max(em, es) / b
    print(f"cohort_stats N={N} M={M} K={K} d={d}: max |mean - ref| = {em:.3e}, max |std - ref| = {es:.3e}, bound {b:.3e}, "
          f"worst ratio {max(em, es) / b:.4f} (so far over all cases: {max(_worst.values()):.4f})")
    assert mean.dtype == np.float32 and std.dtype == np.float32 and mean.shape == (N,) and std.shape == (N,)
    assert em <= b and es <= b
    return E, Cn, mean, std


@pytest.mark.parametrize("N,M,K,d", STAT_CASES)
def test_cohort_stats_against_float64(engine, N, M, K, d):
    check_stats(engine, N, M, K, d, seed=N * 7 + M)


def test_cohort_stats_over_more_than_one_row_block(engine):
    M, K, d = 64, 20, 64
    rb = block_rows(M)
    assert 64 <= rb <= 4096, rb
    N = rb + 37                                                        # the block loop runs twice, the second time with a partial tile
    E, Cn, mean, std = check_stats(engine, N, M, K, d, seed=3)
    m1, s1 = gpu_stats(engine, E[rb - 1:rb + 2], Cn, K)                # the rows around the seam, as a call of their own
    assert np.array_equal(m1, mean[rb - 1:rb + 2]) and np.array_equal(s1, std[rb - 1:rb + 2])
    m0, s0 = engine.cohort_stats(dev(E[:0]), dev(Cn), K)               # N = 0 is a no-op
    assert m0.shape == (0,) and s0.shape == (0,)


# ---- 2. the key mapping and ties ------------------------------------------------------------------------------------------------------
def test_all_scores_negative(engine):
    rng = np.random.default_rng(11)
    d = 192
    e = unit(rng.standard_normal((1, d)))
    Cn = unit(-e + 0.3 * unit(rng.standard_normal((200, d))))          # every cosine below zero
    assert (SR.cosines(e, Cn) < -0.5).all()
    for K in (1, 17, 200):
        mean, std = gpu_stats(engine, e, Cn, K)
        rmean, rstd = SR.cohort_stats(e, Cn, K)
        assert abs(mean[0] - rmean[0]) <= score_bound(d) and abs(std[0] - rstd[0]) <= score_bound(d) and mean[0] < 0


def test_a_run_of_equal_scores_across_the_cut_changes_nothing(engine):
    rng = np.random.default_rng(12)
    d = 192
    E = unit(rng.standard_normal((4, d)))
    hot = unit(E[0] + 0.8 * unit(rng.standard_normal(d)))             # near window 0: its 40 copies sit at the top of that row
    Cn = np.concatenate([unit(rng.standard_normal((100, d))), np.repeat(hot[None], 40, axis=0), unit(rng.standard_normal((60, d)))])
    perm = rng.permutation(len(Cn))
    Cn = np.ascontiguousarray(Cn[perm])
    row0 = np.sort(SR.cosines(E[:1], Cn)[0])[::-1]
    assert abs(row0[39] - SR.cosines(E[:1], hot[None])[0, 0]) < 1e-15 and row0[40] < 0.5 < row0[39]
    stats = {}
    for K in (1, 20, 39, 40, 41, 120):                                 # K cuts through the run, ends it, passes it
        mean, std = gpu_stats(engine, E, Cn, K)
        rmean, rstd = SR.cohort_stats(E, Cn, K)
        assert np.abs(mean - rmean).max() <= score_bound(d) and np.abs(std - rstd).max() <= score_bound(d)
        stats[K] = (mean, std)
    for K in (1, 20, 39, 40):                                          # inside the run the top-K of row 0 is K times one value
        assert stats[K][0][0] == stats[1][0][0] and stats[K][1][0] == STD_FLOOR32
    back = np.argsort(perm)                                            # the multiset has no order: the cohort's row order changes nothing
    m2, s2 = gpu_stats(engine, E, np.ascontiguousarray(Cn[back]), 20)
    assert np.abs(m2 - stats[20][0]).max() <= 2.0 ** -22 and np.abs(s2 - stats[20][1]).max() <= 2.0 ** -22


def test_identical_cohort_rows_give_the_floor_exactly(engine):
    rng = np.random.default_rng(13)
    d = 192
    E = unit(rng.standard_normal((5, d)))
    Cn = np.repeat(unit(rng.standard_normal((1, d))), 300, axis=0)
    for K in (1, 150, 300):
        mean, std = gpu_stats(engine, E, Cn, K)
        assert (std == np.float32(SR.STD_FLOOR)).all()
        assert np.abs(mean - SR.cosines(E, Cn[:1])[:, 0]).max() <= score_bound(d)


# ---- 3. independence and determinism -------------------------------------------------------------------------------------------------
def test_a_rows_statistics_do_not_depend_on_the_other_rows_and_runs_agree_bit_for_bit(engine):
    rng = np.random.default_rng(14)
    N, M, K, d = 70, 1000, 300, 192
    E, Cn = unit(rng.standard_normal((N, d))), unit(rng.standard_normal((M, d)))
    mean, std = gpu_stats(engine, E, Cn, K)
    again = gpu_stats(engine, E, Cn, K)
    assert np.array_equal(again[0], mean) and np.array_equal(again[1], std)
    for n in (0, 31, 32, 63, 64, 69):
        m1, s1 = gpu_stats(engine, E[n:n + 1], Cn, K)
        assert m1[0] == mean[n] and s1[0] == std[n], n
    mt, st = gpu_stats(engine, E, np.ascontiguousarray(Cn[:900]), K)   # another M tail: a statistic of other scores, but still a clean run
    rmean, rstd = SR.cohort_stats(E, Cn[:900], K)
    assert np.abs(mt - rmean).max() <= score_bound(d) and np.abs(st - rstd).max() <= score_bound(d)


# ---- 4. the normalised top-k against the reference -----------------------------------------------------------------------------------
def planted(N, Pn, k, d=192, M=400, K=100, seed=0):
    """Windows = a weighted sum of min(k + 1, Pn) profiles (weights 1, 0.8, 0.6, ..) + noise; profiles = orthonormal directions (no cross-talk
    between the planted ranks); cohort = independent Gaussian directions.  Statistics in float64 from the reference, rounded to fp32 (what
    the kernel reads)."""
    rng = np.random.default_rng(seed)
    P = unit(np.linalg.qr(rng.standard_normal((d, d)))[0].T[:Pn])
    Cn = unit(rng.standard_normal((M, d)))
    m = min(k + 1, Pn)
    E = np.empty((N, d))
    for n in range(N):
        pick = (n + np.arange(m) * 7) % Pn if Pn >= 7 * m else (n + np.arange(m)) % Pn
        E[n] = sum((1.0 - 0.2 * j) * P[p] for j, p in enumerate(pick)) + 0.3 * unit(rng.standard_normal(d))
    E = unit(E)
    me, se = (a.astype(np.float32) for a in SR.cohort_stats(E, Cn, K))
    mp, sp = (a.astype(np.float32) for a in SR.cohort_stats(P, Cn, K))
    return E, P, me, se, mp, sp


def gpu_topk(engine, E, me, se, P, mp, sp, k):
    idx, z, raw = engine.affinity_topk_snorm(dev(E), dev(me), dev(se), dev(P), dev(mp), dev(sp), k=k)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), z.cpu().numpy(), raw.cpu().numpy()


def clear_rows(Z, B, k):
    """Rows whose reference ranking is decided: every gap between consecutive ranked z, down to rank k against rank k + 1, exceeds twice the
    element bound of either neighbour."""
    N, Pn = Z.shape
    ok = np.ones(N, bool)
    for n in range(N):
        order = np.argsort(-Z[n], kind="stable")
        for j in range(min(k, Pn - 1)):
            a, b = order[j], order[j + 1]
            ok[n] &= (Z[n, a] - Z[n, b]) > 2.0 * max(B[n, a], B[n, b])
    return ok


TOPK_CASES = [(33, 1, 1), (70, 100, 1), (70, 100, 4), (70, 3, 3)]      # at d = 192, seed N + Pn + k
# d = 320: the second column of a thread live for wave 0 only; seed 320, for which the reference alone excuses no row (174 excuses one of the 70)
TOPK_WIDE = (70, 100, 4, 320, 320)


def topk_reference(N, Pn, k, d, seed):
    """-> (the planted inputs, SR.topk's tuple, the element bounds B [N, Pn], the rows whose reference ranking is decided)."""
    inputs = planted(N, Pn, k, d, seed=seed)
    E, P, me, se, mp, sp = inputs
    ref = SR.topk(E, me, se, P, mp, sp, k)
    B = 4.0 * score_bound(d) * (1.0 + np.abs(ref[3])) / np.minimum(se.astype(np.float64)[:, None], sp.astype(np.float64)[None, :])
    return inputs, ref, B, clear_rows(ref[3], B, k)


@pytest.mark.parametrize("N,Pn,k", TOPK_CASES)
def test_normalised_topk_against_the_reference(engine, N, Pn, k):
    check_topk(engine, N, Pn, k, 192, N + Pn + k)


def test_normalised_topk_where_the_second_column_is_partly_live(engine):
    """Checked on the CPU (tests/test_snorm_cpu.py prints it): the reference alone excuses 0 of the 70 rows (at most 1 % may be), and without
    the columns 256.. it names other profiles."""
    check_topk(engine, *TOPK_WIDE)


def check_topk(engine, N, Pn, k, d, seed):
    (E, P, me, se, mp, sp), (ridx, rz, rraw, Z, S), B, ok = topk_reference(N, Pn, k, d, seed)
    assert (~ok).sum() <= 0.01 * N, f"the reference alone excuses {(~ok).sum()} of {N} rows"
    if d in PW.WIDTHS:
        SR.second_column_weight_topk(f"snorm topk N={N} Pn={Pn} k={k} d={d}", E, me, se, P, mp, sp, k, (ridx, rz, rraw), float(B.max()))
    idx, z, raw = gpu_topk(engine, E, me, se, P, mp, sp, k)
    assert idx.shape == (N, k) and idx.dtype == np.int32 and z.dtype == np.float32 and raw.dtype == np.float32
    assert np.array_equal(idx[ok], ridx[ok])
    assert (idx >= 0).all() and (idx < Pn).all()
    rows = np.arange(N)[:, None]
    ez, er = np.abs(z - Z[rows, idx]), np.abs(raw - S[rows, idx])                 # every returned entry against the reference AT ITS OWN index
    print(f"snorm topk N={N} Pn={Pn} k={k}: excused rows {(~ok).sum()}, worst |z - ref| / bound = {(ez / B[rows, idx]).max():.4f}, "
          f"worst |raw - ref| / bound = {er.max() / score_bound(d):.4f}")
    assert (ez <= B[rows, idx]).all() and er.max() <= score_bound(d)
    for n in range(N):                                                            # best first, no profile twice
        assert len(set(idx[n].tolist())) == k and all(z[n, j] >= z[n, j + 1] for j in range(k - 1))


def test_exact_ties_go_to_the_lower_index_and_a_nan_window_gets_minus_one(engine):
    d = 192
    E, P, me, se, mp, sp = planted(40, 140, 1, d, seed=9)              # two profile tiles
    for a, b in ((5, 3), (131, 17), (139, 130), (100, 40)):            # a copy of row b (and of its statistics) at row a: same or other tile / thread
        P[a], mp[a], sp[a] = P[b], mp[b], sp[b]
    E[0] = unit(P[3] + 0.1 * E[0])
    E[1] = unit(P[17] + 0.1 * E[1])
    E[2] = unit(P[130] + 0.1 * E[2])
    E[3] = unit(P[40] + 0.1 * E[3])
    E[7, 50] = np.nan
    idx, z, raw = gpu_topk(engine, E, me, se, P, mp, sp, 4)
    assert idx[0, :2].tolist() == [3, 5] and z[0, 0] == z[0, 1] and raw[0, 0] == raw[0, 1]
    assert idx[1, :2].tolist() == [17, 131] and z[1, 0] == z[1, 1]
    assert idx[2, :2].tolist() == [130, 139] and z[2, 0] == z[2, 1]
    assert idx[3, :2].tolist() == [40, 100] and z[3, 0] == z[3, 1]
    assert idx[7].tolist() == [-1] * 4 and z[7].tolist() == [0.0] * 4 and raw[7].tolist() == [0.0] * 4
    assert (idx[np.arange(40) != 7] >= 0).all()
    mp2 = mp.copy()
    mp2[3] = np.nan                                                    # a profile without statistics never wins: its copy takes the slot
    idx2, _, _ = gpu_topk(engine, E, me, se, P, mp2, sp, 1)
    assert idx2[0, 0] == 5 and 3 not in idx2
    mean, std = gpu_stats(engine, E[6:9], unit(np.random.default_rng(1).standard_normal((100, d))), 10)
    assert np.isnan(mean[1]) and np.isnan(std[1]) and np.isfinite(mean[[0, 2]]).all() and np.isfinite(std[[0, 2]]).all()


# ---- 5. the case normalisation exists for --------------------------------------------------------------------------------------------
def knot_case(d=192, seed=21):
    """One window e; profile A at cosine 0.50 inside a dense knot of cohort rows, profile B at cosine 0.48 in an empty region."""
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((d, d)))[0].T
    e, u, v = basis[0], basis[1], basis[2]
    A = 0.50 * e + np.sqrt(1 - 0.50 ** 2) * u
    Bp = 0.48 * e + np.sqrt(1 - 0.48 ** 2) * v
    knot = unit(0.5 * A + np.sqrt(0.75) * unit(rng.standard_normal((300, d - 3)) @ basis[3:]) + 0.01 * rng.standard_normal((300, d)))
    Cn = np.concatenate([knot, unit(rng.standard_normal((100, d)))])
    return unit(e[None]), unit(np.stack([A, Bp])), np.ascontiguousarray(Cn[rng.permutation(len(Cn))])


def test_the_dense_knot_case_raw_takes_a_normalised_takes_b(engine):
    d, K = 192, 100
    E, P, Cn = knot_case(d)
    me, se = SR.cohort_stats(E, Cn, K)
    mp, sp = SR.cohort_stats(P, Cn, K)
    ridx, rz, rraw, Z, S = SR.topk(E, me, se, P, mp, sp, 2)
    zb = 4.0 * score_bound(d) * (1.0 + np.abs(Z)).max() / min(se.min(), sp.min())
    print(f"knot case: cosines {S[0].round(4).tolist()}, top-{K} means e {me[0]:.3f} A {mp[0]:.3f} B {mp[1]:.3f}, stds e {se[0]:.3f} A {sp[0]:.3f} "
          f"B {sp[1]:.3f}, z {Z[0].round(3).tolist()}, element bound {zb:.2e}")
    assert abs(S[0, 0] - 0.50) < 1e-6 and abs(S[0, 1] - 0.48) < 1e-6 and abs(mp[0] - 0.5) < 0.05
    assert ridx[0].tolist() == [1, 0] and Z[0, 1] - Z[0, 0] > 10 * zb, "the reference must prefer B by a wide margin"
    En, Eb, re = engine.l2norm(dev(E))
    Pn, Pb, rp = engine.l2norm(dev(P))
    raw_idx, raw_sc = engine.affinity_topk(En, Eb, re, Pn, Pb, rp.max().reshape(1), k=1)
    mean_e, std_e = engine.cohort_stats(En, dev(Cn), K)
    mean_p, std_p = engine.cohort_stats(Pn, dev(Cn), K)
    idx, z, raw = engine.affinity_topk_snorm(En, mean_e, std_e, Pn, mean_p, std_p, k=2)
    torch.cuda.synchronize()
    assert raw_idx.cpu().numpy()[0, 0] == 0 == int(np.argmax(S[0]))                  # the raw cosine takes A, as the reference's cosines do
    assert idx.cpu().numpy()[0].tolist() == [1, 0]                                    # the normalised score takes B
    assert np.abs(z.cpu().numpy()[0] - rz[0]).max() <= 3 * zb                         # statistics from the device here: their own bound twice more
    assert np.abs(raw.cpu().numpy()[0] - rraw[0]).max() <= 2 * score_bound(d)


# ---- 6. refusals are Python exceptions, and the next call is fine ----------------------------------------------------------------------
def test_refusals_raise_and_leave_the_device_usable(engine):
    rng = np.random.default_rng(31)
    d = 192
    E, Cn, P = dev(unit(rng.standard_normal((6, d)))), dev(unit(rng.standard_normal((50, d)))), dev(unit(rng.standard_normal((8, d))))
    mean, std = engine.cohort_stats(E, Cn, 10)
    mp, sp = engine.cohort_stats(P, Cn, 10)
    good = engine.affinity_topk_snorm(E, mean, std, P, mp, sp, k=2)
    with pytest.raises(ValueError, match="fp32"):
        engine.cohort_stats(E.double(), Cn, 10)
    with pytest.raises(ValueError, match="fp32"):
        engine.cohort_stats(E, Cn.half(), 10)
    with pytest.raises(ValueError, match="contiguous"):
        engine.cohort_stats(dev(unit(rng.standard_normal((6, 2 * d))))[:, ::2], Cn, 10)
    with pytest.raises(ValueError, match="contiguous"):
        engine.affinity_topk_snorm(E, mean, std, P, mp.repeat_interleave(2)[::2], sp, k=1)
    with pytest.raises(ValueError, match="d=96"):
        engine.cohort_stats(E[:, :96].contiguous(), Cn[:, :96].contiguous(), 10)
    with pytest.raises(ValueError, match="d=96"):
        engine.affinity_topk_snorm(E[:, :96].contiguous(), mean, std, P[:, :96].contiguous(), mp, sp, k=1)
    with pytest.raises(ValueError, match="expected 192"):
        engine.cohort_stats(E, Cn[:, :128].contiguous(), 10)
    with pytest.raises(ValueError, match="K=51"):
        engine.cohort_stats(E, Cn, 51)
    with pytest.raises(ValueError, match="K=0"):
        engine.cohort_stats(E, Cn, 0)
    with pytest.raises(ValueError, match="k=5"):
        engine.affinity_topk_snorm(E, mean, std, P, mp, sp, k=5)
    with pytest.raises(ValueError, match="mean_e"):
        engine.affinity_topk_snorm(E, mean[:5], std, P, mp, sp, k=1)
    with pytest.raises(ValueError, match="std_p"):
        engine.affinity_topk_snorm(E, mean, std, P, mp, sp.double(), k=1)
    need = LIB.load_library().sdk_cohort_stats_workspace_bytes(6, 50, 10)
    with pytest.raises(LIB.SdkError, match=f"workspace of {need - 1} bytes, {need} needed"):
        engine.cohort_stats(E, Cn, 10, ws=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    lib, st = engine.lib, torch.cuda.current_stream().cuda_stream      # the same through the C ABI: return codes and messages, nothing launched
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.sdk_cohort_stats(engine.ctx, E.data_ptr(), 6, Cn.data_ptr(), 50, d, 51, mean.data_ptr(), std.data_ptr(), ws.data_ptr(), need, st) == 2
    assert b"K=51" in lib.sdk_last_error()
    assert lib.sdk_cohort_stats(engine.ctx, E.data_ptr(), 6, None, 50, d, 10, mean.data_ptr(), std.data_ptr(), ws.data_ptr(), need, st) == 2
    assert b"null argument" in lib.sdk_last_error()
    m2, s2 = engine.cohort_stats(E, Cn, 10, ws=ws)                     # exactly the bytes the function names are enough
    again = engine.affinity_topk_snorm(E, m2, s2, P, mp, sp, k=2)
    torch.cuda.synchronize()
    assert torch.equal(m2, mean) and torch.equal(s2, std) and all(torch.equal(a, b) for a, b in zip(good, again))


def e2e_z_bound(S, Z, me, se, mp, sp, d):
    """What a device z may differ from the float64 z [N, Pn] by when its statistics are the device's own.  With a = (s - m_e) / s_e and the
    device's s, m_e, s_e off by ds <= d 2^-24 (the fp32 dot) and dm, dsd <= SCORE_BOUND = 2 d 2^-24 (the statistics' bound), the device's a
    is off by ((ds - dm) - a dsd) / (s_e - dsd): at most (1.5 + |a|) SCORE_BOUND / (s_e - SCORE_BOUND); the same for the profile side, half
    the sum of both for z, and |z| 2^-23 for the fp32 rounding of the float64 result."""
    b = score_bound(d)
    a_e, a_p = np.abs((S - me[:, None]) / se[:, None]), np.abs((S - mp[None, :]) / sp[None, :])
    return 0.5 * ((1.5 + a_e) * b / (se[:, None] - b) + (1.5 + a_p) * b / (sp[None, :] - b)) + np.abs(Z) * 2.0 ** -23


# ---- 7. the Backend end to end -------------------------------------------------------------------------------------------------------
def test_backend_identifies_on_the_normalised_scale_and_is_untouched_without_a_cohort(tmp_path, monkeypatch):
    """Synthetic weights and the stand-in voices of evals/run_eval.py --synthesize.  Both sides read the DEVICE's own window, profile and cohort
    rows, so the kernels' arithmetic alone separates the Backend's rows from snorm_ref + the aggregation rule.  The synthetic weights put every
    embedding within a cosine of 0.98 of every other, so the cohort standard deviations are about 1e-3 - 4e-3 and the worst-case fp32 bound
    on a z (e2e_z_bound) is about 0.1 on z values between -4 and 4: some windows' two best profiles lie closer than that, and the comparison
    is built so that they do not decide it (reference()).  The vote threshold is taken from the reference: the middle of the widest gap
    between the sorted top-1 z of the windows; every window's z is asserted to lie at least twice its bound away from it."""
    sys.path.insert(0, str(ROOT / "evals"))
    from run_eval import render_voice
    wav, store, BK = sub("wav"), sub("store"), sub("backend")
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    cohort_path = tmp_path / "cohort.npy"
    monkeypatch.setenv("SDK_COHORT", str(cohort_path))
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "0")
    monkeypatch.delenv("SDK_COHORT_TOPK", raising=False)
    be = BK.Backend()
    eng = be.engine()
    d = be.embedding_dim

    def recording(name, tags, seconds, seed):
        path = tmp_path / f"{name}.wav"
        wav.write_wav_s16(path, np.concatenate([render_voice(t, seconds, seed + 11 * j) for j, t in enumerate(tags)]))
        return path

    profiles = []
    for i, sid in enumerate(("ann", "bob", "cy")):
        rec = be.enroll_speaker(recording(f"enroll_{sid}", [sid], 5.0, 100 + i))
        profiles.append({"id": sid, "names": {"default": sid.title()}, "embeddings": {"mi355x": [
            {"id": f"emb-{sid}", "external_id": rec["external_id"], "model_version": rec["model_version"], "trust_level": "high"}]}})
    imp = [recording(f"impostor_{j}", [f"impostor-{j}"], 4.0, 200 + j) for j in range(7)]
    info = be.make_cohort(imp, cohort_path)
    stored = np.load(cohort_path, allow_pickle=False)
    assert info["n_recordings"] == 7 and stored.shape == (7, d) and stored.dtype == np.float32
    assert np.abs(np.linalg.norm(stored.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(stored[2], be._enroll_vector(imp[2], None)[0])                       # a row is the vector enroll_speaker would store
    co = be.cohort()
    assert len(co) == 7 and co.digest == SN.Cohort(stored, d).digest
    K = 7                                                                                      # min(SDK_COHORT_TOPK = 300, M)

    meeting = recording("meeting", ["bob", "ann", "stranger"], 4.0, 300)
    second = recording("second", ["cy", "ann"], 3.0, 400)
    batch = store.load_profile_batch(profiles, "mi355x", model_prefix="mi355x-")
    Pd = be.profile_tensors(batch)[0]
    Cd = co.device_rows(eng)

    def reference(path, cand_batch, Pdev):
        """The float64 reference on the device's rows, beside the Backend's own per-window answer (score_windows_snorm).  The device's winner
        of a window must be one the bound allows (no other profile's z - bound lies above its z + bound) with its z and raw cosine within
        their bounds; the reference's z and raw AT THAT PROFILE are what the aggregation rule is then applied to, so a window whose two
        best z lie closer than the arithmetic can tell apart (the gap rule of the top-k test) does not decide the comparison."""
        samples, starts, W, spans = be._windows(path, None)
        Ed = be.embed_tables(samples, {W: starts})[W][0]
        E, P, Cn = Ed.cpu().numpy(), Pdev.cpu().numpy(), Cd.cpu().numpy()
        me, se = SR.cohort_stats(E, Cn, K)
        mp, sp = SR.cohort_stats(P, Cn, K)
        ridx, rz, _, Z, S = SR.topk(E, me, se, P, mp, sp, 1)
        assert min(se.min(), sp.min()) > 2 * score_bound(d), "the bound's denominator"
        ZB = e2e_z_bound(S, Z, me, se, mp, sp, d)
        didx, dz, draw = (a[:, 0] for a in be.score_windows_snorm(Ed, cand_batch))
        n = np.arange(len(E))
        assert (didx >= 0).all() and (didx < P.shape[0]).all()
        zsel, zbsel, rawsel = Z[n, didx], ZB[n, didx], S[n, didx]
        assert (np.abs(dz - zsel) <= zbsel).all() and (np.abs(draw - rawsel) <= score_bound(d)).all()
        assert ((Z - ZB).max(axis=1) <= zsel + zbsel).all(), "the device's winner must be one the bound allows"
        print(f"e2e snorm {path.name}: {len(E)} windows x {P.shape[0]} profiles, std_e {se.min():.2e} .. {se.max():.2e}, std_p {sp.min():.2e} .. {sp.max():.2e}; "
              f"worst |z - ref| / bound {float((np.abs(dz - zsel) / zbsel).max()):.4f}, worst bound {float(ZB.max()):.3e}, "
              f"{int((didx != ridx[:, 0]).sum())} winners differ from the reference's inside the bound")
        return didx, zsel, rawsel, zbsel, rz[:, 0], spans

    def same_rows(rows, want, zb):
        """Backend rows against the aggregation rule's, speaker by speaker (the order is the rows' own norm_score: two speakers whose reference
        norm_score lie within the bound of each other may stand either way round)."""
        assert rows == sorted(rows, key=lambda r: (-r["norm_score"], r["speaker_id"]))
        assert sorted(r["speaker_id"] for r in rows) == sorted(r["speaker_id"] for r in want)
        by = {r["speaker_id"]: r for r in rows}
        for w in want:
            r = by[w["speaker_id"]]
            assert set(r) >= {"speaker_id", "similarity", "confidence", "norm_score", "embedding_id", "segment", "n_segments"}
            assert r["n_segments"] == w["n_segments"] and r["embedding_id"] == w["embedding_id"] and r["segment"] == w["segment"]
            assert abs(r["similarity"] - w["similarity"]) <= score_bound(d) and r["confidence"] == r["similarity"]     # the mean of the RAW cosines
            assert abs(r["norm_score"] - w["norm_score"]) <= zb and -1.0 <= r["similarity"] <= 1.0
        for x, y in zip(want, want[1:]):
            if x["norm_score"] - y["norm_score"] > 2 * zb:
                assert [r["speaker_id"] for r in rows].index(x["speaker_id"]) < [r["speaker_id"] for r in rows].index(y["speaker_id"])

    idx, z, raw, zb, rz, spans = reference(meeting, batch, Pd)
    zs = np.sort(rz)
    g = int(np.argmax(np.diff(zs)))
    thr = float(0.5 * (zs[g] + zs[g + 1]))
    print(f"e2e snorm: top-1 z per window {rz.round(2).tolist()}, threshold {thr:.3f} in a gap of {zs[g + 1] - zs[g]:.3f}, "
          f"least |z - threshold| / bound {float((np.abs(z - thr) / zb).min()):.1f}")
    assert len(z) >= 6 and (np.abs(z - thr) > 2 * zb).all(), "every window's vote must be decided: twice its bound away from the threshold"
    assert (z >= thr).any() and (z < thr).any()
    be.cohort_threshold = thr
    want = SR.aggregate(idx, z, raw, spans, batch.speaker_ids, batch.embedding_ids, thr)
    rows = be.identify_speaker(meeting, profiles, threshold=0.99)                              # the raw threshold is not applied on this path
    assert len(want) >= 1
    same_rows(rows, want, float(zb.max()))
    assert getattr(be.last_batch, "_snorm")[1] == (co.digest, K)                               # the profile statistics are cached on the batch

    many = be.identify_many([meeting, second], profiles)
    assert many == [rows, be.identify_speaker(second, profiles)]

    one = store.load_profile_batch([profiles[0]], "mi355x", model_prefix="mi355x-")
    ridx, vz, vraw, vzb, _, rspans = reference(meeting, one, be.profile_tensors(one)[0])
    vwant = SR.aggregate(ridx, vz, vraw, rspans, one.speaker_ids, one.embedding_ids, thr)
    got = be.verify_speaker(meeting, profiles[0])
    hit = be.identify_speaker(meeting, [profiles[0]])
    if hit:
        assert got == {"match": True, "similarity": hit[0]["similarity"], "confidence": hit[0]["similarity"], "embedding_id": "emb-ann",
                       "norm_score": hit[0]["norm_score"]}
    else:
        assert got == {"match": False, "similarity": 0.0, "confidence": 0.0, "embedding_id": None}
    if (np.abs(vz - thr) > vzb).all():
        same_rows(hit, vwant, float(vzb.max()))

    # with the three variables unset the raw path answers as before: score_windows + aggregate_matches on the same embeddings
    for v in ("SDK_COHORT", "SDK_COHORT_THRESHOLD", "SDK_COHORT_TOPK"):
        monkeypatch.delenv(v, raising=False)
    plain = BK.Backend()
    assert plain.cohort() is None
    samples, starts, W, spans = plain._windows(meeting, None)
    E, Eb, re = plain.embed_tables(samples, {W: starts})[W]
    b2 = store.load_profile_batch(profiles, "mi355x", model_prefix="mi355x-")
    pidx, psc = plain.score_windows(E, Eb, re, b2)
    before = BK.aggregate_matches(pidx[:, 0], psc[:, 0], spans, b2, 0.354)
    now = plain.identify_speaker(meeting, profiles, threshold=0.354)
    assert now == before and all("norm_score" not in r for r in now)
    assert getattr(plain.last_batch, "_snorm", None) is None
