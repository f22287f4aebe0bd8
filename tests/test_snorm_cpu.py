"""CPU checks of the adaptive score normalisation's host side: snorm.py's numpy restatements against the independent float64 reference
(tests/snorm_ref.py), the cohort file's refusals, the Backend's configuration refusals, the aggregation of normalised winners, and the new
C-ABI entry points' host-only answers (workspace size; shape refusals, which come before any device call)."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snorm_ref as SR  # noqa: E402
from conftest import sub  # noqa: E402

SN = sub("snorm")
LIB = sub("_lib")
BK = sub("backend")


def unit(x):
    x = np.asarray(x, dtype=np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def test_std_floor_is_the_rules():
    assert SN.STD_FLOOR == SR.STD_FLOOR == 1e-6


@pytest.mark.parametrize("N,M,K,d", [(1, 64, 1, 64), (9, 257, 100, 192), (5, 300, 300, 192), (4, 300, 299, 128)])
def test_cohort_stats_host_equals_the_reference(N, M, K, d):
    rng = np.random.default_rng(N + M + K)
    E, Cn = unit(rng.standard_normal((N, d))), unit(rng.standard_normal((M, d)))
    Cn[M // 2:M // 2 + 7] = Cn[0]                                     # a run of equal scores for the cut to pass through
    mean, std = SN.cohort_stats_host(E, Cn, K)
    rmean, rstd = SR.cohort_stats(E, Cn, K)
    assert mean.dtype == np.float64 and np.abs(mean - rmean).max() <= 1e-12 and np.abs(std - rstd).max() <= 1e-12


def test_cohort_stats_host_floors_the_std_and_refuses_bad_k():
    e = unit(np.ones((2, 64)))
    Cn = np.repeat(unit(np.arange(1, 65.0)[None]), 10, axis=0)
    mean, std = SN.cohort_stats_host(e, Cn, 4)
    assert (std == SN.STD_FLOOR).all() and np.abs(mean - SR.cosines(e, Cn)[:, 0]).max() <= 1e-15
    for K in (0, 11):
        with pytest.raises(ValueError, match="K="):
            SN.cohort_stats_host(e, Cn, K)


@pytest.mark.parametrize("N,Pn,k", [(7, 1, 1), (20, 30, 1), (20, 30, 4), (6, 3, 3)])
def test_snorm_topk_host_equals_the_reference(N, Pn, k):
    rng = np.random.default_rng(100 + Pn + k)
    E, P, Cn = unit(rng.standard_normal((N, 64))), unit(rng.standard_normal((Pn, 64))), unit(rng.standard_normal((50, 64)))
    if Pn >= 3:
        P[2] = P[0]                                                   # an exact tie: identical rows, identical statistics
    me, se = SR.cohort_stats(E, Cn, 20)
    mp, sp = SR.cohort_stats(P, Cn, 20)
    idx, z, raw = SN.snorm_topk_host(E, me, se, P, mp, sp, k)
    ridx, rz, rraw, _, _ = SR.topk(E, me, se, P, mp, sp, k)
    assert idx.dtype == np.int32 and np.array_equal(idx, ridx)
    assert np.abs(z - rz).max() <= 1e-12 and np.abs(raw - rraw).max() <= 1e-12
    if Pn >= 3:
        assert not (idx == 2)[(idx == 0).any(axis=1)][:, 0].any()     # of the tied pair the lower index comes first


def test_snorm_topk_host_nan_never_wins():
    rng = np.random.default_rng(5)
    E, P, Cn = unit(rng.standard_normal((3, 64))), unit(rng.standard_normal((4, 64))), unit(rng.standard_normal((20, 64)))
    E[1, 3] = np.nan
    me, se = SR.cohort_stats(E, Cn, 5)
    mp, sp = SR.cohort_stats(P, Cn, 5)
    mp[2] = np.nan                                                    # one profile without statistics: it never appears
    idx, z, raw = SN.snorm_topk_host(E, me, se, P, mp, sp, 4)
    ridx, rz, rraw, _, _ = SR.topk(E, me, se, P, mp, sp, 4)
    assert np.array_equal(idx, ridx) and np.abs(z - rz).max() <= 1e-12 and np.abs(raw - rraw).max() <= 1e-12
    assert idx[1].tolist() == [-1] * 4 and z[1].tolist() == [0.0] * 4 and raw[1].tolist() == [0.0] * 4
    assert 2 not in idx and idx[0, 3] == -1 and z[0, 3] == 0.0 and raw[0, 3] == 0.0
    with pytest.raises(ValueError, match="k=5"):
        SN.snorm_topk_host(E, me, se, P, mp, sp, 5)


# ---- the GPU cases at a partly live second column --------------------------------------------------------------------------------------
def test_the_gpu_cases_at_320_and_448_weigh_the_second_column_and_excuse_no_more_rows():
    """What tests/test_snorm_gpu.py asserts on the reference alone before it asks the device at d = 320 and 448: without the columns 256.. the
    statistics move by more than 100 x their bound and the top-k names other profiles; the reference excuses at most 1 % of the top-k rows."""
    import partial_width as PW
    import test_snorm_gpu as SG                                       # its cases and generators; importing it needs no GPU
    stats = [c for c in SG.STAT_CASES if c[3] in PW.WIDTHS]
    assert {c[3] for c in stats} == set(PW.WIDTHS)
    for N, M, K, d in stats:
        E, Cn = SG.stats_rows(N, M, d, N * 7 + M)
        assert SR.second_column_weight_stats(f"cohort_stats N={N} M={M} K={K} d={d}", E, Cn, K, SR.cohort_stats(E, Cn, K), SG.score_bound(d)) > PW.FAR
    assert SG.TOPK_WIDE[:4] == (70, 100, 4, 320)
    for N, Pn, k, d, seed in [SG.TOPK_WIDE]:
        (E, P, me, se, mp, sp), ref, B, ok = SG.topk_reference(N, Pn, k, d, seed)
        print(f"snorm topk N={N} Pn={Pn} k={k} d={d}: the reference alone excuses {int((~ok).sum())} of {N} rows (at most {0.01 * N:g})")
        assert (~ok).sum() <= 0.01 * N
        assert SR.second_column_weight_topk(f"snorm topk N={N} Pn={Pn} k={k} d={d}", E, me, se, P, mp, sp, k, ref[:3], float(B.max())) > PW.FAR


# ---- the cohort file -----------------------------------------------------------------------------------------------------------------
def test_cohort_loads_a_good_file_and_carries_a_content_digest(tmp_path):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((5, 192)).astype(np.float32)
    np.save(tmp_path / "c.npy", a)
    co = SN.Cohort.load(tmp_path / "c.npy", 192)
    assert len(co) == 5 and co.dim == 192 and np.array_equal(co.matrix, a) and len(co.digest) == 16
    b = a.copy()
    b[3, 7] += 1.0
    assert SN.Cohort(b, 192).digest != co.digest and SN.Cohort(a.copy(), 192).digest == co.digest


def test_cohort_refuses_each_bad_file(tmp_path):
    rng = np.random.default_rng(1)
    good = rng.standard_normal((4, 192)).astype(np.float32)

    def load(name, arr, dim=192):
        np.save(tmp_path / name, arr)
        return SN.Cohort.load(tmp_path / name, dim)

    with pytest.raises(ValueError, match="rank 1"):
        load("rank1.npy", good[0])
    with pytest.raises(ValueError, match="rank 3"):
        load("rank3.npy", good[None])
    with pytest.raises(ValueError, match="d=192.*embedding_dim is 256"):
        load("dim.npy", good, 256)
    bad = good.copy()
    bad[2, 5] = np.inf
    with pytest.raises(ValueError, match="row 2 holds a non-finite"):
        load("inf.npy", bad)
    bad = good.copy()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="row 1 holds a non-finite"):
        load("nan.npy", bad)
    bad = good.copy()
    bad[3] = 0.0
    with pytest.raises(ValueError, match="row 3 is a zero row"):
        load("zero.npy", bad)
    big = np.lib.format.open_memmap(tmp_path / "big.npy", mode="w+", dtype=np.float32, shape=((1 << 20) + 1, 64))     # sparse: never filled
    del big
    with pytest.raises(ValueError, match=r"M=1048577 rows"):
        SN.Cohort.load(tmp_path / "big.npy", 64)
    with pytest.raises(ValueError, match="M=0 rows"):
        load("empty.npy", np.zeros((0, 192), np.float32))
    np.save(tmp_path / "obj.npy", np.array([{"a": 1}], dtype=object), allow_pickle=True)
    with pytest.raises(ValueError, match="not a readable .npy"):                                  # a pickled payload is never executed
        SN.Cohort.load(tmp_path / "obj.npy", 192)


# ---- Backend configuration -----------------------------------------------------------------------------------------------------------
def _clear(monkeypatch):
    for v in ("SDK_COHORT", "SDK_COHORT_TOPK", "SDK_COHORT_THRESHOLD", "SDK_NO_TORCH"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("SDK_ECAPA_WEIGHTS", "unused.npz")             # only silences the synthetic-weights notice; nothing is loaded here


def test_backend_refuses_a_cohort_without_a_threshold(monkeypatch):
    _clear(monkeypatch)
    monkeypatch.setenv("SDK_COHORT", "cohort.npy")
    with pytest.raises(ValueError, match="SDK_COHORT .*SDK_COHORT_THRESHOLD"):
        BK.Backend()
    _clear(monkeypatch)
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "2.5")
    with pytest.raises(ValueError, match="SDK_COHORT .*SDK_COHORT_THRESHOLD"):
        BK.Backend()
    monkeypatch.setenv("SDK_COHORT", "cohort.npy")
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "high")
    with pytest.raises(ValueError, match="SDK_COHORT_THRESHOLD='high'"):
        BK.Backend()


def test_backend_refuses_a_cohort_on_the_torch_free_path(monkeypatch):
    _clear(monkeypatch)
    monkeypatch.setenv("SDK_COHORT", "cohort.npy")
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "2.5")
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    with pytest.raises(ValueError, match="SDK_NO_TORCH=1.*torch engine"):
        BK.Backend()


def test_backend_reads_the_cohort_settings(monkeypatch):
    _clear(monkeypatch)
    be = BK.Backend()
    assert be.cohort_path is None and be.cohort_threshold is None and be.cohort() is None
    monkeypatch.setenv("SDK_COHORT", "cohort.npy")
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "-1.25")
    be = BK.Backend()
    assert be.cohort_path == "cohort.npy" and be.cohort_threshold == -1.25 and be.cohort_topk == 300
    monkeypatch.setenv("SDK_COHORT_TOPK", "0")
    with pytest.raises(ValueError, match="SDK_COHORT_TOPK=0"):
        BK.Backend()


# ---- aggregation ---------------------------------------------------------------------------------------------------------------------
class _Batch:
    speaker_ids = ["ann", "bob", "ann", "cy"]
    embedding_ids = ["a0", "b0", "a1", "c0"]


def test_aggregation_votes_on_z_takes_similarity_from_raw_and_sorts_by_norm_score():
    idx = np.array([0, 2, 1, 1, -1, 3, 2], np.int32)
    z = np.array([3.0, 5.0, 9.0, 1.9, 50.0, 2.0, np.nan], np.float32)
    raw = np.array([0.9, 0.7, 0.2, 0.99, 0.99, -0.1, 0.8], np.float32)
    spans = [(float(w), float(w) + 2.0) for w in range(7)]
    rows = BK.aggregate_matches_snorm(idx, z, raw, spans, _Batch, 2.0)
    assert [r["speaker_id"] for r in rows] == ["bob", "ann", "cy"]                     # by norm_score 9, 4, 2 - not by similarity 0.2, 0.8, -0.1
    bob, ann, cy = rows
    assert bob["norm_score"] == 9.0 and bob["n_segments"] == 1                          # z = 1.9 < 2 does not vote although its cosine is 0.99
    assert bob["similarity"] == bob["confidence"] == float(np.float32(0.2))
    assert ann["norm_score"] == 4.0 and ann["similarity"] == float(np.mean(np.array([np.float32(0.9), np.float32(0.7)], np.float64)))
    assert ann["embedding_id"] == "a0" and ann["segment"] == (0.0, 3.0) and ann["n_segments"] == 2
    assert cy["norm_score"] == 2.0 and cy["similarity"] == float(np.float32(-0.1))      # z == threshold votes; a negative cosine is no obstacle
    assert rows == SR.aggregate(idx, z, raw, spans, _Batch.speaker_ids, _Batch.embedding_ids, 2.0)
    assert BK.aggregate_matches_snorm(idx, z, raw, spans, _Batch, 100.0) == []
    tie = BK.aggregate_matches_snorm(np.array([3, 1], np.int32), np.array([4.0, 4.0], np.float32), np.array([0.1, 0.9], np.float32), spans[:2], _Batch, 0.0)
    assert [r["speaker_id"] for r in tie] == ["bob", "cy"]                              # equal norm_score: by speaker id


# ---- the C ABI, host-only ------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_and_the_abi_version_stays():
    lib = LIB.load_library()
    for name in ("sdk_cohort_stats_workspace_bytes", "sdk_cohort_stats", "sdk_affinity_topk_snorm"):
        assert hasattr(lib, name) and name in LIB.SIGNATURES
    assert lib.sdk_abi_version() == 4


def test_workspace_bytes_is_positive_monotone_in_m_and_bounded_in_n():
    lib = LIB.load_library()
    ws = lib.sdk_cohort_stats_workspace_bytes
    for N in (0, 1, 1000, 1 << 30):
        for M in (1, 64, 2000, 10000, 100000, 1 << 20):
            assert ws(N, M, 1) > 0 and ws(N, M, M) > 0
    for N in (1, 70, 1000, 1 << 30):
        sizes = [ws(N, M, 1) for M in (1, 63, 64, 65, 2000, 10000, 100000, 1 << 20)]
        assert sizes == sorted(sizes), (N, sizes)
    for M in (64, 10000, 100000, 1 << 20):
        cap = ws(1 << 30, M, 1)
        assert ws((1 << 31) - 1, M, 1) == cap and ws(1 << 20, M, 1) == cap             # row blocks: no growth with N beyond one block
        assert cap <= max(256 << 20, 64 * M * 4 + 256)
        grow = [ws(N, M, 1) for N in (1, 2, 64, 65, 1024, 1025, 5000)]
        assert grow == sorted(grow) and grow[-1] <= cap
    assert ws(1000, 0, 1) == 0 and b"M=0" in lib.sdk_last_error()
    assert ws(1000, (1 << 20) + 1, 1) == 0 and b"M=1048577" in lib.sdk_last_error()
    assert ws(1000, 100, 0) == 0 and b"K=0" in lib.sdk_last_error()
    assert ws(1000, 100, 101) == 0 and b"K=101" in lib.sdk_last_error()
    assert ws(-1, 100, 1) == 0 and b"N=-1" in lib.sdk_last_error()


def test_shape_refusals_come_before_any_device_call():
    """No device here and no context: every call below must fail on its shape check (rc 2, the value named), not on the null context."""
    lib = LIB.load_library()

    def stats(M, d, K):
        return lib.sdk_cohort_stats(None, None, 4, None, M, d, K, None, None, None, 0, None)

    def topk(d, k, Pn=10):
        return lib.sdk_affinity_topk_snorm(None, None, None, None, 4, None, None, None, Pn, d, k, None, None, None, None)

    assert stats(100, 96, 10) == 2 and b"d=96" in lib.sdk_last_error()
    assert stats(100, 576, 10) == 2 and b"d=576" in lib.sdk_last_error()
    assert stats(100, 192, 0) == 2 and b"K=0" in lib.sdk_last_error()
    assert stats(100, 192, 101) == 2 and b"K=101" in lib.sdk_last_error()
    assert stats((1 << 20) + 1, 192, 10) == 2 and b"M=1048577" in lib.sdk_last_error()
    assert topk(192, 5) == 2 and b"k=5" in lib.sdk_last_error()
    assert topk(192, 0) == 2 and b"k=0" in lib.sdk_last_error()
    assert topk(96, 1) == 2 and b"d=96" in lib.sdk_last_error()
    assert topk(192, 1, Pn=0) == 2 and b"Pn=0" in lib.sdk_last_error()
    assert stats(100, 192, 10) == 2 and b"null context" in lib.sdk_last_error()         # good shapes: only then the context is looked at
    assert topk(192, 1) == 2 and b"null context" in lib.sdk_last_error()
