"""CPU checks of the speaker-count bounds (`speakers=`): the option's parsing, the bounds' target, the one-pass level search of
cluster.agglomerative_cluster rule 7 against a brute-force reference (one flat partition per level), and the k-means restatement that the GPU
tests compare the kernel with (tests/kmeans_ref.py)."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ahc_ref as AHC  # noqa: E402
import kmeans_ref as KR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
cluster = importlib.import_module(f"{PKG}.cluster")
dz = importlib.import_module(f"{PKG}.diarize")


def unit_rows(seed: int, N: int, d: int = 16, groups: int = 4) -> np.ndarray:
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((groups, d))
    X = cen[rng.integers(0, groups, N)] + 0.35 * rng.standard_normal((N, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


_LINK = {}


def linkage(seed: int, N: int):
    if (seed, N) not in _LINK:
        X = unit_rows(seed, N)
        _LINK[(seed, N)] = (X, AHC.centroid_linkage(X)[0])
    return _LINK[(seed, N)]


# ------------------------------------------------------------------------------------------------ options
def test_speakers_parsing_and_refusals():
    assert cluster.parse_speakers(None) is None
    assert cluster.parse_speakers(1) == (1, 1) and cluster.parse_speakers(np.int64(3)) == (3, 3)
    assert cluster.parse_speakers((2, 5)) == (2, 5) and cluster.parse_speakers([2, 2]) == (2, 2)
    assert cluster.parse_speakers((None, 4)) == (1, 4) and cluster.parse_speakers((2, None)) == (2, None)
    assert cluster.parse_speakers((None, None)) == (1, None)
    for bad in (0, -1, (3, 2), "2", (0, 2), (1, 2, 3), 2.0, True, (1.0, 2), ("1", 2), {}, (2,)):
        with pytest.raises(ValueError, match="speakers="):
            cluster.parse_speakers(bad, "here")
    d = dz.Diarizer(None, None, None)                                     # no engine: the refusal comes before any device work
    for bad in (0, (3, 2), "2"):
        with pytest.raises(ValueError, match="speakers="):
            d.run(np.zeros(16000, np.int16), speakers=bad)
        with pytest.raises(ValueError, match="speakers="):
            d.run_many([np.zeros(16000, np.int16)], speakers=bad)
    assert d._check_options("x", "ahc", None, None) == ({}, None) and d._check_options("x", "ahc", None, None, 2) == ({}, (2, 2))


def test_target_rule():
    t = cluster.speaker_target
    assert t(3, None, 100) is None and t(3, (1, None), 100) is None and t(3, (3, 3), 100) is None and t(3, (2, 5), 100) is None
    assert t(3, (4, 6), 100) == 4 and t(3, (1, 2), 100) == 2 and t(3, (5, None), 100) == 5
    assert t(3, (50, 60), 7) == 7 and t(1, (2, 2), 1) is None and t(1, (2, 2), 0) is None and t(1, (2, 2), 2) == 2
    for found, lo, hi, n in ((3, 4, 6, 100), (3, None, 2, 100), (3, 2, None, 100), (9, 1, 1, 5), (1, 2, 2, 1)):
        assert t(found, cluster.parse_speakers((lo, hi)), n) == KR.target_of(found, lo, hi, n)
    assert dz.DiarizationResult.forced is None and cluster.VbxResult.forced is None and cluster.AgglomerativeResult.forced is None
    assert "forced" not in dz.DiarizationResult.__dataclass_fields__


# ------------------------------------------------------------------------------------------------ the level search against brute force
@pytest.mark.parametrize("N", [2, 3, 11, 120, 121])
@pytest.mark.parametrize("eff", [1, 12])
def test_level_search_against_brute_force(N, eff):
    X, Z = linkage(N, N)
    L = cluster.level_counts(Z, eff)
    brute = [int((np.bincount(cluster._flat_partition(Z, N, t)) >= eff).sum()) for t in range(N)]
    assert L.tolist() == brute == KR.level_counts(Z, eff) and L.shape == (N,)
    assert np.abs(np.diff(L)).max(initial=0) <= 1 and (L[-1] == 1 or eff > N)       # unit steps down to one cluster
    for q in (0.25, 0.5, 0.9):
        thr = float(np.quantile(Z[:, 2], q))
        t0 = cluster.cut_level(Z, thr)
        assert t0 == KR.cut_merges(Z, thr) and np.array_equal(cluster.fcluster_distance(Z, thr), AHC.partition_after(Z, N, t0))
        K0 = max(int(L[t0]), 1)
        for target in sorted({1, 2, max(K0 - 1, 1), K0 + 1, N}):
            target = min(target, N)
            got, count = cluster.level_search(Z, eff, t0, target)
            want = KR.level_search_brute(Z, eff, t0, target, cluster._flat_partition)
            assert got == want == KR.level_search(Z, eff, t0, target) and count == L[got]
            if target <= K0 and L[t0] >= 1:
                assert count == target                                    # every target <= K0 is reachable
            if eff == 1:
                assert count == target and got == N - target


def test_level_search_with_an_inversion_and_an_unreachable_target():
    seed = next(s for s in range(100) if AHC.inversions(linkage(1000 + s, 40)[1]) > 0)
    X, Z = linkage(1000 + seed, 40)
    assert AHC.inversions(Z) > 0
    for eff in (1, 4):
        for t0 in (0, 10, 25, 39):
            for target in (1, 2, 5, 17, 40):
                assert cluster.level_search(Z, eff, t0, target)[0] == KR.level_search_brute(Z, eff, t0, target, cluster._flat_partition)
    X, Z = linkage(120, 120)
    L = cluster.level_counts(Z, 12)
    assert L.max() < 120 // 12 + 1 <= 120                                 # fewer than target clusters of 12 rows at any level
    got, count = cluster.level_search(Z, 12, cluster.cut_level(Z, float(np.median(Z[:, 2]))), 120)
    assert count == L.max() and got == KR.level_search_brute(Z, 12, cluster.cut_level(Z, float(np.median(Z[:, 2]))), 120, cluster._flat_partition)


# ------------------------------------------------------------------------------------------------ agglomerative_cluster on a stub provider
class StubProvider:
    """centroid_linkage from the reference, nothing else: agglomerative_cluster's host logic alone."""

    def __init__(self):
        self.calls = 0

    def centroid_linkage(self, E):
        self.calls += 1
        return torch.from_numpy(AHC.centroid_linkage(E.numpy().astype(np.float64))[0])


@pytest.mark.parametrize("N,mcs", [(11, 2), (60, 3), (60, 12)])
def test_agglomerative_cluster_with_and_without_speakers(N, mcs):
    X = unit_rows(7 + N, N)
    E = torch.from_numpy(X.astype(np.float32))
    Z = AHC.centroid_linkage(X)[0]
    thr = float(np.quantile(Z[:, 2], 0.8))
    p = StubProvider()
    base = cluster.agglomerative_cluster(p, E, thr, mcs)
    none = cluster.agglomerative_cluster(p, E, thr, mcs, speakers=None)
    want = AHC.threshold_rule(Z, X, thr, mcs)
    assert np.array_equal(base.labels, want) and np.array_equal(none.labels, want) and base.forced is None and none.forced is None
    assert base.n_large == none.n_large and np.array_equal(base.linkage, none.linkage)
    K0 = int(want.max()) + 1
    inside = cluster.agglomerative_cluster(p, E, thr, mcs, speakers=(max(K0 - 1, 1), K0 + 1))
    assert np.array_equal(inside.labels, want) and inside.forced is None
    for sp, lo, hi in ((1, 1, 1), (2, 2, 2), (K0 + 1, K0 + 1, K0 + 1), ((K0 + 2, None), K0 + 2, None), ((None, max(K0 - 1, 1)), None, max(K0 - 1, 1))):
        res = cluster.agglomerative_cluster(p, E, thr, mcs, speakers=sp)
        ref, forced = KR.ahc_bounded(Z, X, thr, mcs, lo, hi)
        assert np.array_equal(res.labels, ref)
        if forced is None:
            assert res.forced is None and np.array_equal(res.labels, want)
            continue
        assert res.forced == {k: forced[k] for k in ("found", "target", "method", "level", "n_iter")} and res.forced["found"] == K0
        if forced["reachable"]:
            assert int(res.labels.max()) + 1 == forced["target"] == res.n_large
    with pytest.raises(ValueError, match="speakers="):
        cluster.agglomerative_cluster(p, E, thr, mcs, speakers=0)
    with pytest.raises(ValueError, match="pass one"):
        cluster.agglomerative_cluster(p, E, thr, mcs, n_clusters=2, speakers=2)
    one = cluster.agglomerative_cluster(p, E[:1], thr, mcs, speakers=3)
    assert one.labels.tolist() == [0] and one.forced is None              # fewer than two rows: nothing is forced


# ------------------------------------------------------------------------------------------------ the k-means restatement itself
def planted(seed: int, N: int, d: int, k: int, noise: float) -> np.ndarray:
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((k, d))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    X = cen[rng.integers(0, k, N)] + noise * rng.standard_normal((N, d)) / np.sqrt(d)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def test_kmeans_restatement_finds_planted_clusters_and_states_its_order():
    E = planted(3, 300, 64, 3, 0.5)
    r = KR.kmeans(E, 3)
    assert r["n_clusters"] == 3 and 2 <= r["n_iter"] < 20 and r["counts"].sum() == 300 and r["least"] > 1e-6
    assert np.array_equal(r["labels"], KR.kmeans(E, 3, max_iters=40)["labels"])
    assert np.allclose(np.linalg.norm(r["cent64"], axis=1), 1.0, atol=1e-15)
    X = E.astype(np.float64)
    assert KR.seeds(X, 1) == [0] and KR.seeds(X, 3)[0] == 0 and len(set(KR.seeds(X, 3))) == 3
    # the sums: segment partials in segment order, not one running sum
    big = planted(4, 2500, 64, 2, 0.5).astype(np.float64)
    lab = (np.arange(2500) % 2).astype(np.int64)
    s, cnt = KR.sums_in_order(big, lab, 2)
    parts = [np.cumsum(big[t0:t0 + 1024][lab[t0:t0 + 1024] == 0], axis=0)[-1] for t0 in (0, 1024, 2048)]
    assert np.array_equal(s[0], (parts[0] + parts[1]) + parts[2]) and cnt.tolist() == [1250, 1250]
    # two identical rows at k = 2: both seeds are row 0, every tie goes to the lower centre, one cluster is left
    two = KR.kmeans(np.stack([E[0], E[0]]), 2)
    assert two["labels"].tolist() == [0, 0] and two["n_clusters"] == 1
    with pytest.raises(ValueError):
        KR.kmeans(np.full((3, 64), np.nan, np.float32), 2)


# ------------------------------------------------------------------------------------------------ the GPU cases at partly live second columns
def _kmeans_gpu_cases():
    import test_kmeans_gpu as KG                                              # its cases and generators; importing it needs no GPU
    return KG


@pytest.mark.parametrize("case", ["one-step-%d-%d-%d" % c for c in _kmeans_gpu_cases().PARTIAL_ONE_STEP] + ["whole-loop"])
def test_the_kmeans_cases_at_320_and_448_decide_every_row_and_weigh_the_second_column(case):
    """What tests/test_kmeans_gpu.py asserts on the restatement alone before it asks the device, at d = 320 and 448: the least margin over
    10 x the bound with no row left out, and other labels (or centres 100 x their bound away) without the columns 256..."""
    KG = _kmeans_gpu_cases()
    if case == "whole-loop":
        N, d, k, seed, noise = KG.PARTIAL_LOOP
        E, kw = KG.planted(seed, N, d, k, noise), {}
    else:
        N, d, k = (int(v) for v in case.split("-")[2:])
        E, kw = KG.one_step_rows(N, d), dict(max_iters=1)
    ref = KR.kmeans(E, k, **kw)
    bound = KG.kmeans_bound(d)
    left_out = int(sum((m <= 10 * bound).sum() for m in ref["margins"]))
    print(f"kmeans {case} N={N} d={d} k={k}: least margin {ref['least']:.3e} over {ref['n_iter']} assignments (10 x bound {10 * bound:.3e}); rows left out {left_out}; "
          f"clusters {ref['n_clusters']}")
    assert d in KR.PW.WIDTHS and ref["least"] > 10 * bound and left_out == 0
    assert ref["n_iter"] == 1 if kw else 2 <= ref["n_iter"] < cluster.KMEANS_MAX_ITERS
    assert KR.second_column_weight(f"kmeans {case}", E, k, (d + 4) * 2.0 ** -53, ref, **kw) > KR.PW.FAR
