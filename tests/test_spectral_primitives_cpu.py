"""The float64 references of tests/spectral_ref.py checked on the CPU: against tests/cpu_provider.py and numpy on random data, and for
the conditions tests/test_spectral_primitives_gpu.py relies on (enough decisive rows per label case; every integer-exact case really is
exact in fp32).  No GPU."""
import numpy as np
import pytest
import torch

import spectral_ref as sr
from conftest import sub
from cpu_provider import CpuProvider

CL = sub("cluster")
P = CpuProvider()
SMALL = [(1, 1), (5, 3), (40, 7), (300, 16), (257, 32)]


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.parametrize("n,k", SMALL)
def test_gram_apply_unit_match_the_cpu_provider_and_numpy(n, k):
    seed = sr.case_seed(n, k)
    X, Y, R = sr.real_rows(n, k, seed), sr.real_rows(n, k, seed + 1), sr.real_rows(k, k, seed + 2)
    sc = np.random.default_rng(seed + 3).uniform(-2, 2, n).astype(np.float32)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    G = sr.gram(X, Y)
    want = X64.T @ Y64
    tol = 4 * n * 2.0 ** -53 * (np.abs(X64).T @ np.abs(Y64)) + 1e-300          # two float64 orders of one sum
    assert (np.abs(G - want) <= tol).all()
    assert np.abs(G - P.rows_gram(t(X), t(Y)).double().numpy()).max() <= 2.0 ** -23 * np.abs(want).max()      # the provider returns fp32
    for scale in (None, sc):
        A = sr.apply(X, R, scale)
        wantA = (X64 @ R.astype(np.float64)) * (1.0 if scale is None else scale.astype(np.float64)[:, None])
        mag = (np.abs(X64) @ np.abs(R.astype(np.float64))) * (1.0 if scale is None else np.abs(scale.astype(np.float64))[:, None])
        assert (np.abs(A - wantA) <= 4 * k * 2.0 ** -53 * mag + 1e-300).all()
        got = P.rows_apply(t(X), t(R), None if scale is None else t(scale)).double().numpy()
        assert (np.abs(A - got) <= 2.0 ** -23 * mag + 1e-300).all()
    U = sr.unit(X)
    assert np.abs(np.linalg.norm(U, axis=1) - 1.0).max() <= 1e-15
    assert np.abs(U - X64 / np.linalg.norm(X64, axis=1, keepdims=True)).max() <= 1e-15
    assert np.abs(U - P.rows_unit(t(X)).double().numpy()).max() <= 2.0 ** -24


def test_unit_floor_and_zero_row():
    X = np.zeros((3, 4), dtype=np.float32)
    X[1] = [3e-20, 0, 4e-20, 0]                                   # norm 5e-20 < 1e-12: divided by the floor, not normalised
    X[2] = [3, 0, 4, 0]
    U = sr.unit(X)
    assert not U[0].any()
    assert np.allclose(U[1], X[1].astype(np.float64) / 1e-12, rtol=1e-15, atol=0)
    assert np.allclose(U[2], [0.6, 0, 0.8, 0], rtol=1e-15, atol=0)


@pytest.mark.parametrize("n,k,kc", [(1, 1, 1), (7, 3, 9), (300, 16, 5), (257, 32, 32)])
def test_assign_and_mindist_match_the_cpu_provider_and_numpy(n, k, kc):
    R, C = sr.label_case(n, k, kc)
    lab, d2, margin = sr.assign(R, C)
    dist = ((R[:, None, :].astype(np.float64) - C[None].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(lab, dist.argmin(1))
    assert np.allclose(d2, dist.min(1), rtol=1e-14, atol=0)
    srt = np.sort(dist, axis=1)
    assert np.allclose(margin, srt[:, 1] - srt[:, 0], rtol=1e-9, atol=1e-13) if kc > 1 else np.isinf(margin).all()
    plab, pd2, ps, pc = P.kmeans_assign(t(R), t(C))
    assert np.array_equal(lab, plab.numpy())
    assert np.allclose(d2, pd2.double().numpy(), rtol=2.0 ** -23, atol=0)
    # the fp32 block sums against the provider's float64 sums: fp32 chains of at most 256 terms
    bs, bc = sr.block_sums_f32(R, lab, kc)
    assert np.array_equal(bc.sum(0), pc.numpy()[0])
    assert np.array_equal(bc.sum(0), np.bincount(lab, minlength=kc))
    absum = np.stack([np.abs(R[lab == q].astype(np.float64)).sum(0) for q in range(kc)])
    assert (np.abs(bs.astype(np.float64).sum(0) - ps.double().numpy()[0]) <= 257 * sr.U24 * absum + 1e-30).all()
    for first in (True, False):
        prev = np.random.default_rng(n).uniform(0, 2 * k, n).astype(np.float32)
        m = sr.mindist(R, C[0], prev, first)
        want = dist[:, 0] if first else np.minimum(prev.astype(np.float64), dist[:, 0])
        assert np.allclose(m, want, rtol=1e-14, atol=0)
        got = P.kmeans_mindist(t(R), t(C[0]), t(prev.copy()), first).double().numpy()
        assert np.allclose(m, got, rtol=2.0 ** -23, atol=0)


def test_assign_breaks_ties_downward_and_gives_a_nan_row_minus_one():
    C = np.array([[0, 0], [2, 0], [2, 0], [0, 0]], dtype=np.float32)          # centres 0 == 3 and 1 == 2
    R = np.array([[1, 0], [0, 0], [2, 0], [np.nan, 0], [1, 5]], dtype=np.float32)
    lab, d2, margin = sr.assign(R, C)
    assert lab.tolist() == [0, 0, 1, -1, 0]
    assert d2[:3].tolist() == [1.0, 0.0, 0.0] and np.isinf(d2[3]) and d2[4] == 26.0
    assert margin[:3].tolist() == [0.0, 0.0, 0.0] and np.isnan(margin[3])
    ps, pc = sr.block_sums_f32(R, lab, 4)
    assert pc.tolist() == [[3, 1, 0, 0]]
    assert ps[0].tolist() == [[2.0, 5.0], [2.0, 0.0], [0.0, 0.0], [0.0, 0.0]]     # the NaN row is in no sum


def test_block_sums_are_one_fp32_chain_in_row_order():
    """Chosen so that the order shows: 2^24 + 1 + 1 stays 2^24 in fp32 when the ones come after, and is 2^24 + 2 when they come first."""
    big = np.float32(2.0 ** 24)
    lab = np.zeros(3, dtype=np.int32)
    assert sr.block_sums_f32(np.array([[big], [1], [1]], dtype=np.float32), lab, 1)[0][0, 0, 0] == big
    assert sr.block_sums_f32(np.array([[1], [1], [big]], dtype=np.float32), lab, 1)[0][0, 0, 0] == big + np.float32(2)
    # a block boundary restarts the chain: row 256 is alone in the second block
    R = np.ones((257, 1), dtype=np.float32)
    ps, pc = sr.block_sums_f32(R, np.zeros(257, dtype=np.int32), 2)
    assert ps[:, :, 0].tolist() == [[256.0, 0.0], [1.0, 0.0]] and pc.tolist() == [[256, 0], [1, 0]]


@pytest.mark.parametrize("k", [1, 2, 5, 31])
@pytest.mark.parametrize("shift_rel", [0.0, 1e-5, 1e-2])
def test_chol_inverse_matches_numpy(k, shift_rel):
    Y = np.random.default_rng(k).standard_normal((200, k))
    G = (Y.T @ Y).astype(np.float32)
    G[0, k - 1] += np.float32(1e-3)
    X, piv, diag = sr.chol_inverse(G, shift_rel)
    G64 = G.astype(np.float64)
    A = 0.5 * (G64 + G64.T) + shift_rel * np.trace(G64) / k * np.eye(k)
    L = np.linalg.cholesky(A)
    want = np.linalg.inv(L.T)
    assert np.abs(X - want).max() <= 1e-12 * np.abs(want).max()
    assert np.allclose(piv, np.diag(L) ** 2, rtol=1e-12, atol=0) and np.allclose(diag, np.diag(A), rtol=1e-15, atol=0)
    assert not np.tril(X, -1).any()
    if shift_rel == 0.0:
        got = P.chol_inverse(t(G)).double().numpy()
        assert np.abs(X - got).max() <= 2.0 ** -23 * np.abs(want).max()


# ------------------------------------------------------------------ the conditions the GPU file relies on
@pytest.mark.parametrize("n,k,kc", sr.NKC_CASES)
def test_label_cases_keep_enough_decisive_rows(n, k, kc):
    """For every (shape, seed) whose labels the GPU file compares, the reference alone keeps at least 95 % of the rows under the margin rule
    (float64 best-minus-second margin > twice the dist2 bound)."""
    R, C = sr.label_case(n, k, kc)
    lab, d2, margin = sr.assign(R, C)
    keep = sr.decisive(k, d2, margin)
    assert (lab >= 0).all()
    assert keep.mean() >= 0.95, (n, k, kc, float(keep.mean()))


def test_case_lists_cover_what_the_issue_names():
    for cases in (sr.NK_CASES, [c[:2] for c in sr.NKC_CASES]):
        assert (257, 32) in cases and (1, 1) in cases
        assert {n for n, _ in cases} == set(sr.N_SET) and {k for _, k in cases} == set(sr.K_SET)
    assert {kc for _, _, kc in sr.NKC_CASES} == set(sr.KC_SET)
    assert any(k == 32 and kc == 32 for _, k, kc in sr.NKC_CASES) and any(kc > n for n, _, kc in sr.NKC_CASES)
    assert 10 <= len(sr.NK_CASES) <= 14 and 10 <= len(sr.NKC_CASES) <= 14


@pytest.mark.parametrize("n,k", sr.NK_CASES)
def test_integer_cases_are_exact_in_fp32(n, k):
    """Every partial sum of the integer-exact cases of rows_gram, rows_apply and kmeans_mindist is an integer (times a power of two)
    below 2^24 in magnitude, so every fp32 fmaf chain is exact whatever its order."""
    seed = sr.case_seed(n, k)
    X, Y, R = sr.int_rows(n, k, seed), sr.int_rows(n, k, seed + 1), sr.int_rows(k, k, seed + 2)
    c = sr.int_rows(1, k, seed + 3)[0]
    for a in (X, Y, R, c):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= sr.INT_MAX
    assert sr.gram(np.abs(X), np.abs(Y)).max() < 2 ** 24
    assert sr.apply(np.abs(X), np.abs(R)).max() < 2 ** 24
    assert sr.mindist(np.abs(X), -np.abs(c), None, True).max() < 2 ** 24
    sc = sr.pow2_scale(n, seed + 4)
    m, e = np.frexp(np.abs(sc))
    assert (m == 0.5).all() and (e >= -2).all() and (e <= 4).all()                  # 2^-3 .. 2^3
    # and the float64 reference of an integer case is an integer (an eighth of one with the scale)
    Yr = sr.apply(X, R, sc) * 8
    assert np.array_equal(Yr, np.round(Yr))


@pytest.mark.parametrize("n,k,kc", sr.NKC_CASES)
def test_integer_label_cases_are_exact_in_fp32(n, k, kc):
    R, C = sr.int_label_case(n, k, kc)
    worst = max(sr.mindist(np.abs(R), -np.abs(C[q]), None, True).max() for q in range(kc))
    assert worst < 2 ** 24
    _, d2, _ = sr.assign(R, C)
    assert np.array_equal(d2, np.round(d2))


# ------------------------------------------------------------------ a negative label
def test_canonical_labels_refuses_a_negative_label_and_names_the_row():
    """kmeans_assign labels a row -1 when it holds a NaN; remap[-1] used to give such a row the last cluster's label without a word."""
    with pytest.raises(ValueError, match=r"row 3 .*label -1"):
        CL.canonical_labels(np.array([2, 2, 0, -1, 1, -1], dtype=np.int32))
    assert CL.canonical_labels(np.array([2, 2, 0, 1], dtype=np.int32)).tolist() == [0, 0, 1, 2]
