"""CPU checks of the constrained assignment's host restatement (diarize.assign_constrained_host) against the all-maps reference of
tests/assign_ref.py and scipy's linear_sum_assignment, and of the reference's two loop forms against each other."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref as AR  # noqa: E402
from conftest import sub  # noqa: E402

dz = sub("diarize")


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def test_reference_forms_agree_and_equal_scipy():
    """chunk_plain (every map in a plain loop) against chunk_axes (first candidate looped, the others as numpy axes) and scipy's optimum;
    half of the tables are small integers, so exact ties occur."""
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(0)
    ties = 0
    for t in range(400):
        m, K = int(rng.integers(1, 4)), int(rng.integers(1, 9))
        cos = rng.integers(0, 4, (m, K)).astype(np.float64) if t % 2 else rng.standard_normal((m, K))
        lab, tot, margin = AR.chunk_plain(cos.tolist())
        r, c = linear_sum_assignment(cos, maximize=True)
        assert tot == pytest.approx(cos[r, c].sum(), abs=1e-12)
        assert sum(k >= 0 for k in lab) == min(m, K) and margin >= 0
        ties += margin == 0
        if K >= m >= 2:
            lab2, tot2, margin2 = AR.chunk_axes(cos)
            assert lab2 == lab and tot2 == tot and margin2 == pytest.approx(margin, abs=1e-15)
        assert dz.constrained_chunk(cos) == lab
    assert ties > 20


@pytest.mark.parametrize("K", [1, 2, 3, 5, 40])
def test_host_equals_the_all_maps_reference(K):
    """(1) labels and centroids on seeded inputs with 0 - 3 candidates per chunk and NaN in every row that is no candidate; the total of
    every chunk is scipy's optimum."""
    from scipy.optimize import linear_sum_assignment
    E, info, train, tl = AR.make_case(10 + K, 60, K)
    assert np.isnan(E).any() and set(np.bincount(AR.assign(E, info, train, tl, constrained=False)["m"], minlength=4).nonzero()[0]) == {0, 1, 2, 3}
    ref = AR.assign(E, info, train, tl)
    labels, cent = dz.assign_constrained_host(E, info, train, tl)
    assert labels.dtype == np.int32 and labels.shape == (info.shape[0], 3) and cent.dtype == np.float32
    assert np.array_equal(labels, ref["labels"])
    assert np.abs(cent.astype(np.float64) - ref["centroids"]).max() <= 2.0 ** -24
    assert ref["bites"][:60].mean() >= 0.1 and ref["margin"].min() > 1e-9
    for c in range(info.shape[0]):
        slots = np.flatnonzero(ref["labels"][c] >= 0)
        cand = [s for s in range(3) if info[c, s, 3] != 0 and info[c, s, 0] > 0]
        assert len(slots) == min(len(cand), K) and len(set(ref["labels"][c, slots])) == len(slots)
        if cand:
            cos = E[3 * c + np.array(cand)].astype(np.float64) @ ref["centroids"].T
            r, k = linear_sum_assignment(cos, maximize=True)
            assert ref["total"][c] == pytest.approx(cos[r, k].sum(), abs=1e-12)


def test_no_training_row_and_no_candidate():
    E, info, _, _ = AR.make_case(3, 20, 4)
    E, info = E[:60], info[:20]
    none = np.zeros(0, np.int64)
    ref = AR.assign(E, info, none, none.astype(np.int32))
    labels, cent = dz.assign_constrained_host(E, info, none, none.astype(np.int32))
    assert cent.shape == (1, 192) and np.array_equal(labels, ref["labels"]) and np.abs(cent - ref["centroids"]).max() <= 2.0 ** -24
    assert (np.sort(labels[ref["m"] >= 2], axis=1)[:, :2] == -1).all() and ((labels >= 0).sum(1) == np.minimum(ref["m"], 1)).all()
    info0 = np.zeros_like(info)
    labels, cent = dz.assign_constrained_host(E, info0, none, none.astype(np.int32))
    assert cent.shape == (0, 192) and (labels == -1).all()


@pytest.mark.parametrize("K", [3, 7])
def test_constraint_that_does_not_bite_equals_assign_rows(K):
    """(2) K >= 3 and no two candidates of a chunk share their nearest centroid: exactly assign_rows."""
    E, info, train, tl = AR.make_case(20 + K, 80, K, p_bite=0.0)
    E = np.nan_to_num(E)                                                 # assign_rows reads every row
    ref = AR.assign(E, info, train, tl)
    keep = ~ref["bites"]
    keep[0] = False                                                      # make_case's chunk 0 always bites
    info = info.copy()
    info[~keep] = 0
    assert keep.sum() > 40
    la, ca = dz.assign_rows(E, info, train, tl)
    lb, cb = dz.assign_constrained_host(E, info, train, tl)
    assert np.array_equal(la, lb) and np.array_equal(ca, cb)


def tie_case(K=4):
    """One chunk whose candidates in slots 0 and 2 are bitwise the same row, nearest to centroid 2, then 1."""
    rng = np.random.default_rng(5)
    cen = unit(rng.standard_normal((K, 192)))
    row = unit(cen[2] + 0.5 * cen[1] + 0.02 * rng.standard_normal(192))
    E = np.full((3 + 3 * K, 192), np.nan, np.float32)
    info = np.zeros((1 + K, 3, 4), np.int32)
    E[0] = E[2] = row
    info[0, 0] = info[0, 2] = (100, 50, 1, 1)
    for k in range(K):
        E[3 + 3 * k] = cen[k]
        info[1 + k, 0] = (300, 300, 1, 1)
    return E, info, np.arange(3, 3 + 3 * K, 3), np.arange(K, dtype=np.int32)


def few_centroids_case():
    """One centroid, three candidates; slots 0 and 2 hold the same row (the largest cosine), slot 1 a farther one."""
    rng = np.random.default_rng(6)
    cen = unit(rng.standard_normal((1, 192)))
    near, far = unit(cen[0] + 0.3 * unit(rng.standard_normal(192))), unit(cen[0] + 0.9 * unit(rng.standard_normal(192)))
    E = np.stack([near, far, near, cen[0], cen[0] * 0, cen[0] * 0]).astype(np.float32)
    info = np.zeros((2, 3, 4), np.int32)
    info[0] = (100, 50, 1, 1)
    info[1, 0] = (300, 300, 1, 1)
    return E, info, np.array([3]), np.zeros(1, np.int32)


def test_exact_ties():
    """(3) two candidates that are bitwise the same row: slot 0 gets the lower of the two best clusters, slot 1 the other."""
    E, info, train, tl = tie_case()
    labels, _ = dz.assign_constrained_host(E, info, train, tl)
    assert labels[0].tolist() == [1, -1, 2]
    assert np.array_equal(labels, AR.assign(E, info, train, tl)["labels"])
    assert dz.assign_rows(np.nan_to_num(E), info, train, tl)[0][0].tolist() == [2, -1, 2]


def test_fewer_centroids_than_candidates():
    """(4) one centroid, three candidates: the candidate of largest cosine keeps it (lowest slot on a tie), the others are dropped."""
    E, info, train, tl = few_centroids_case()
    labels, cent = dz.assign_constrained_host(E, info, train, tl)
    assert labels[0].tolist() == [0, -1, -1] and cent.shape == (1, 192)
    assert np.array_equal(labels, AR.assign(E, info, train, tl)["labels"])
    E[[0, 1]] = E[[1, 0]]                                                # the far row first: the best cosine is now in slots 1 and 2
    assert dz.assign_constrained_host(E, info, train, tl)[0][0].tolist() == [-1, 0, -1]


def test_result_has_scores_last():
    r = dz.DiarizationResult([], 0, None, None, None, None, None, None)
    assert r.cls is None and r.scores is None
    assert list(dz.DiarizationResult.__dataclass_fields__)[-2:] == ["cls", "scores"]
    import inspect
    assert inspect.signature(dz.Diarizer.run).parameters["constrained"].default is False
