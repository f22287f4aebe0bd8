"""CPU checks of the VBx clustering's host side: the loop-form reference (tests/vbx_ref.py) against a second, vectorised form; the PLDA
preparation (plda.prepare) against scipy.linalg.eigh; the .npz round trip; the rule's edge cases on the reference; the new C-ABI symbols."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbx_ref as VR  # noqa: E402
from conftest import sub  # noqa: E402

P = sub("plda")
LIB = sub("_lib")


def case(seed, N, d_in, D, S, n_true, D0=128):
    m = P.synthetic_plda(d_in, D0, seed=seed, lda_dim=D)
    Phi_full, T_full = P.prepare(m.tr, m.psi, D0)
    E, rows, init, true = VR.mixture(seed + 1, N, d_in, D0, D, S, n_true, (m.mean1, m.lda, m.mean2, m.mu, Phi_full), T_full)
    return m, E, rows, init, true


def vbx_vectorised(X, Phi, init, S, Fa=0.07, Fb=0.8, max_iters=20, epsilon=1e-4, init_smoothing=7.0):
    """The same rule with matrix products and numpy's own (pairwise) sums."""
    from scipy.special import logsumexp, softmax
    n, D = X.shape
    rho = X * np.sqrt(Phi)
    G = -0.5 * ((X ** 2).sum(1) + D * np.log(2 * np.pi))
    gamma = softmax(init_smoothing * (np.arange(S)[None, :] == np.asarray(init)[:, None]), axis=1)
    pi = np.full(S, 1.0 / S)
    elbo = []
    for ii in range(max_iters):
        invL = 1.0 / (1.0 + Fa / Fb * gamma.sum(0)[:, None] * Phi)
        alpha = Fa / Fb * invL * (gamma.T @ rho)
        logp = Fa * (rho @ alpha.T - 0.5 * ((invL + alpha ** 2) @ Phi)[None, :] + G[:, None])
        with np.errstate(divide="ignore"):
            z = logp + np.log(pi)
        lse = logsumexp(z, axis=1)
        gamma = np.exp(z - lse[:, None])
        elbo.append(lse.sum() + 0.5 * Fb * (np.log(invL) - invL - alpha ** 2 + 1).sum())
        pi = gamma.sum(0) / gamma.sum()
        if ii > 0 and elbo[-1] - elbo[-2] < epsilon:
            break
    return gamma, pi, np.array(elbo)


@pytest.mark.parametrize("N,d_in,D,S,n_true", [(63, 256, 64, 7, 3), (150, 192, 128, 20, 4)])
def test_reference_equals_the_vectorised_form(N, d_in, D, S, n_true):
    m, E, rows, init, true = case(3, N, d_in, D, S, n_true)
    X = VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T)
    assert np.abs(X - m.transform_host(E[rows])).max() <= 1e-12 * np.abs(X).max()
    ref = VR.vbx(X, m.Phi, init, S)
    gamma, pi, elbo = vbx_vectorised(X, m.Phi, init, S)
    assert ref["n_iter"] == len(elbo) and 2 <= len(elbo)
    assert np.abs(ref["gamma"] - gamma).max() <= 1e-11 and np.abs(ref["pi"] - pi).max() <= 1e-12
    assert np.abs(ref["elbo"] - elbo).max() <= 1e-10 * np.abs(elbo).max()
    res = VR.result(ref["gamma"], ref["pi"], E[rows])
    K = len(res["keep"])
    assert n_true <= K < S                                               # speakers died out
    g = gamma[:, res["keep"]]
    cent = (g.T @ E[rows].astype(np.float64)) / g.sum(0)[:, None]
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    assert np.abs(res["cent"] - cent).max() <= 1e-13 and np.array_equal(res["labels"], np.argmax(g, axis=1))
    # the kept speakers recover the true ones: every row sits with the rows of its own speaker
    for k in range(K):
        assert len(set(true[res["labels"] == k])) <= 1
    # long double and the descending row order change nothing that is decided
    for kw in (dict(dtype=np.longdouble), dict(reverse=True)):
        alt = VR.vbx(VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T, kw.get("dtype", np.float64)), m.Phi, init, S, **kw)
        assert alt["n_iter"] == ref["n_iter"] and float(np.abs(alt["gamma"] - ref["gamma"]).max()) <= 1e-12


def test_preparation_against_scipy():
    import scipy.linalg
    rng = np.random.default_rng(5)
    D0 = 96
    tr = rng.standard_normal((D0, D0)) / np.sqrt(D0) + 0.8 * np.eye(D0)    # a general, well-conditioned matrix
    psi = np.sort(rng.uniform(0.05, 20.0, D0))[::-1]
    Phi, T = P.prepare(tr, psi, 64)
    W = np.linalg.inv(tr.T @ tr)
    B = np.linalg.inv((tr.T / psi) @ tr)
    lam, V = scipy.linalg.eigh(B, W)
    lam, V = lam[::-1], V[:, ::-1]
    assert Phi.shape == (64,) and T.shape == (64, D0) and (np.diff(Phi) < 0).all()
    assert np.abs(Phi - lam[:64]).max() <= 1e-9 * lam[0]
    sign = np.sign((T * V.T[:64]).sum(1))
    assert np.abs(T - sign[:, None] * V.T[:64]).max() <= 1e-8
    assert np.abs(T @ W @ T.T - np.eye(64)).max() <= 1e-9
    # the synthetic model: psi positive descending, well conditioned, Phi = psi
    m = P.synthetic_plda(192, 128, 0)
    assert (m.psi > 0).all() and (np.diff(m.psi) < 0).all() and np.linalg.cond(m.tr) < 2.1 and m.lda_dim == 128
    assert np.abs(m.Phi - m.psi).max() <= 1e-9 * m.psi[0] and np.abs(m.T @ np.linalg.inv(m.tr.T @ m.tr) @ m.T.T - np.eye(128)).max() <= 1e-9
    m2 = P.synthetic_plda(192, 128, 0)
    assert np.array_equal(m.lda, m2.lda) and np.array_equal(m.T, m2.T)


def test_npz_round_trip_and_refusals(tmp_path):
    m = P.synthetic_plda(256, 128, 7)
    np.savez(tmp_path / "xvec_transform.npz", mean1=m.mean1, mean2=m.mean2, lda=m.lda)
    np.savez(tmp_path / "plda.npz", mu=m.mu, tr=m.tr, psi=m.psi)
    for D in (64, 128):
        got = P.load_plda(tmp_path / "xvec_transform.npz", tmp_path / "plda.npz", lda_dim=D)
        assert got.lda_dim == D and got.d_in == 256 and got.D0 == 128
        for k in ("mean1", "mean2", "lda", "mu", "tr", "psi"):
            assert np.array_equal(getattr(got, k), getattr(m, k))
        assert np.array_equal(got.Phi, m.Phi[:D]) and np.array_equal(got.T, m.T[:D])
    np.savez(tmp_path / "bad.npz", mu=m.mu, tr=m.tr)
    with pytest.raises(ValueError, match="lacks"):
        P.load_plda(tmp_path / "xvec_transform.npz", tmp_path / "bad.npz")
    with pytest.raises(ValueError, match="lda_dim=96"):
        P.load_plda(tmp_path / "xvec_transform.npz", tmp_path / "plda.npz", lda_dim=96)
    with pytest.raises(ValueError, match="d_in=100"):
        P.Plda(np.zeros(100), np.zeros((100, 64)), np.zeros(64), np.zeros(64), np.eye(64), np.ones(64), 64)
    with pytest.raises(ValueError, match="psi"):
        P.Plda(np.zeros(128), np.zeros((128, 64)), np.zeros(64), np.zeros(64), np.eye(64), -np.ones(64), 64)


def test_a_dying_speaker_gets_gamma_exactly_zero():
    m, E, rows, init, _ = case(11, 63, 192, 64, 7, 3)
    X = VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T)
    ref = VR.vbx(X, m.Phi, init, 7, max_iters=60, epsilon=-np.inf)
    dead = np.flatnonzero(ref["pi"] == 0.0)
    assert ref["n_iter"] == 60 and len(dead) >= 1, ref["pi"]
    assert not ref["gamma"][:, dead].any()                               # exactly 0, not merely small
    assert np.isfinite(ref["elbo"]).all() and np.isfinite(ref["gamma"]).all() and abs(ref["pi"].sum() - 1.0) <= 1e-12
    res = VR.result(ref["gamma"], ref["pi"], E[rows])
    assert not set(dead.tolist()) & set(res["keep"].tolist()) and res["labels"].max() < len(res["keep"])


def test_one_speaker_and_two_rows():
    m, E, rows, init, _ = case(13, 2, 192, 64, 1, 1)
    X = VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T)
    ref = VR.vbx(X, m.Phi, np.zeros(2, np.int32), 1)
    assert ref["n_iter"] == 2 and np.array_equal(ref["gamma"], np.ones((2, 1))) and ref["pi"].tolist() == [1.0]
    res = VR.result(ref["gamma"], ref["pi"], E[rows])
    mean = E[rows].astype(np.float64).sum(0) / 2
    assert res["keep"].tolist() == [0] and res["labels"].tolist() == [0, 0] and np.abs(res["cent"][0] - mean / np.linalg.norm(mean)).max() <= 1e-15
    two = VR.vbx(X, m.Phi, np.array([0, 1], np.int32), 2)
    assert two["gamma"].shape == (2, 2) and abs(two["pi"].sum() - 1.0) <= 1e-15 and np.isfinite(two["elbo"]).all()


def test_the_new_symbols_are_exported_and_host_entry_points_answer():
    lib = LIB.load_library()
    for name in ("sdk_plda_transform", "sdk_vbx_workspace_bytes", "sdk_vbx", "sdk_vbx_centroids"):
        assert hasattr(lib, name) and name in LIB.SIGNATURES
    n, D, S = 2049, 128, 130
    nblk = -(-n // 64)
    assert lib.sdk_vbx_workspace_bytes(n, D, S) >= 8 * (n * D + nblk * S * (D + 1))
    assert lib.sdk_vbx_workspace_bytes(n, 96, S) == 0 and b"D=96" in lib.sdk_last_error()
    assert lib.sdk_vbx_workspace_bytes(n, D, 0) == 0 and lib.sdk_vbx_workspace_bytes(65537, D, S) == 0


def test_unknown_clustering_is_refused_before_any_device_work():
    dz = sub("diarize")
    d = dz.Diarizer(None, None, None)
    with pytest.raises(ValueError, match="clustering='spectral'"):
        d.run(np.zeros(16000, np.int16), clustering="spectral")
    with pytest.raises(ValueError, match="vbx="):
        d.run(np.zeros(16000, np.int16), clustering="vbx", vbx={"loop_prob": 0.9})
    with pytest.raises(ValueError, match="vbx="):
        d.run(np.zeros(16000, np.int16), vbx={"Fa": 0.1})
    r = dz.DiarizationResult([], 0, None, None, None, None, None, None)
    assert r.pi is None and r.elbo is None and r.scores is None
    assert sub("cluster").VBX_AHC_THRESHOLD == 0.6
