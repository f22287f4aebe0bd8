"""CPU checks of VBx with its HMM on the host side: the loop-form reference (tests/vbx_hmm_ref.py) against an independent dense
forward-backward; against the mixture reference at loop_prob = 0; what the loop probability is for (isolated single frames stay with their
neighbours); the log domain where probabilities would underflow; the new symbols and keywords."""
from __future__ import annotations

import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbx_hmm_ref as HR  # noqa: E402
import vbx_ref as VR  # noqa: E402
from conftest import sub  # noqa: E402

P = sub("plda")
LIB = sub("_lib")
MARGIN, ULPS = 8.0, 4.0


def case(seed, N, d_in, D, S, n_true, D0=128):
    """A mixture laid out in speaker runs -> (model, X [N, D] float64 in time order, init [N], true [N])."""
    m = P.synthetic_plda(d_in, D0, seed=seed, lda_dim=D)
    Phi_full, T_full = P.prepare(m.tr, m.psi, D0)
    E, rows, init, true = VR.mixture(seed + 1, N, d_in, D0, D, S, n_true, (m.mean1, m.lda, m.mean2, m.mu, Phi_full), T_full)
    order = HR.speaker_runs(true, np.random.default_rng(seed + 2))
    X = VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T)
    return m, X[order], init[order], true[order]


def dense_forward_backward(logp, pi, loop_prob, dtype=np.float64, reverse=False, fn=None):
    """The textbook form: an explicit S x S transition matrix, probabilities scaled per row, matrix products."""
    n, S = logp.shape
    tr = loop_prob * np.eye(S) + (1.0 - loop_prob) * np.tile(pi, (S, 1))
    shift = logp.max(1)
    b = np.exp(logp - shift[:, None])
    a = np.zeros((n, S))
    c = np.zeros(n)
    a[0] = pi * b[0]
    c[0] = a[0].sum()
    a[0] /= c[0]
    for t in range(1, n):
        a[t] = (a[t - 1] @ tr) * b[t]
        c[t] = a[t].sum()
        a[t] /= c[t]
    be = np.ones((n, S))
    for t in range(n - 2, -1, -1):
        be[t] = tr @ (b[t + 1] * be[t + 1]) / c[t + 1]
    gamma = a * be
    tll = np.log(c).sum() + shift.sum()
    # the expected number of times a speaker is ENTERED from pi: row 0, and the (1 - P) pi_j part of every transition into j
    pinew = gamma[0].copy()
    for t in range(1, n):
        pinew += a[t - 1].sum() * (1.0 - loop_prob) * pi * b[t] * be[t] / c[t]
    return dict(lf=None, lb=None, m=None, tll=tll, gamma=gamma, pinew=pinew)


@pytest.mark.parametrize("loop_prob", [0.0, 0.5, 0.99])
def test_reference_equals_a_dense_forward_backward(loop_prob):
    m, X, init, true = case(3, 40, 192, 64, 5, 3)
    ref = HR.vbx_hmm(X, m.Phi, init, 5, loop_prob)
    den = HR.vbx_hmm(X, m.Phi, init, 5, loop_prob, fb=dense_forward_backward)
    print(f"P={loop_prob}: n_iter {ref['n_iter']} / {den['n_iter']}, max|d gamma| {np.abs(ref['gamma'] - den['gamma']).max():.2e}, "
          f"max|d pi| {np.abs(ref['pi'] - den['pi']).max():.2e}, max|d elbo| {np.abs(ref['elbo'] - den['elbo']).max():.2e}")
    assert ref["n_iter"] == den["n_iter"] >= 2
    assert np.abs(ref["gamma"] - den["gamma"]).max() <= 1e-11 and np.abs(ref["pi"] - den["pi"]).max() <= 1e-12
    assert np.abs(ref["elbo"] - den["elbo"]).max() <= 1e-11 * np.abs(den["elbo"]).max()
    assert np.abs(ref["gamma"].sum(1) - 1.0).max() <= 1e-11 and abs(ref["pi"].sum() - 1.0) <= 1e-14
    # gamma = exp(lf + lb - tll) is what the chain's two arrays say
    assert ref["lf"].shape == ref["lb"].shape == (40, 5) and not ref["lb"][-1].any()


@pytest.mark.parametrize("N,d_in,D,S,n_true", [(63, 256, 64, 7, 3), (150, 192, 128, 20, 4)])
def test_loop_prob_zero_is_the_mixture(N, d_in, D, S, n_true):
    """At P = 0 the chain is vbx_ref.vbx in another arithmetic (lf + lb - tll cancels sums of the size of tll).  Within the project's
    8 x yardstick + 4 ulp, the yardstick being the larger of the HMM reference's distance to its long-double and to its reversed run."""
    m, X, init, true = case(5, N, d_in, D, S, n_true)
    mix = VR.vbx(X, m.Phi, init, S)
    runs = {k: HR.vbx_hmm(X, m.Phi, init, S, 0.0, dtype=dt, reverse=rev) for k, dt, rev in (("f64", np.float64, False), ("ld", np.longdouble, False),
                                                                                           ("rev", np.float64, True))}
    assert runs["f64"]["n_iter"] == mix["n_iter"] == runs["ld"]["n_iter"] == runs["rev"]["n_iter"]
    for q in ("gamma", "pi", "elbo"):
        a = runs["f64"][q].astype(np.longdouble)
        y = max(float(np.abs(a - runs[o][q].astype(np.longdouble)).max()) for o in ("ld", "rev"))
        err = float(np.abs(runs["f64"][q] - mix[q]).max())
        tol = MARGIN * y + ULPS * float(np.spacing(np.abs(mix[q]).max()))
        print(f"  {q:6s} max|d| {err:.3e}  yardstick {y:.3e}  tolerance {tol:.3e}")
        assert err <= tol, q


def planted(seed=5, D=64, run=30, n_runs=9):
    """Three speakers taking turns in runs of 30 frames; the frame in the middle of every run belongs to the NEXT speaker."""
    rng = np.random.default_rng(seed)
    Phi = np.geomspace(16.0, 0.05, D)
    means = rng.standard_normal((3, D)) * np.sqrt(Phi)
    around = np.repeat(np.arange(n_runs) % 3, run)
    n = len(around)
    out = np.arange(run // 2, n, run)
    true = around.copy()
    true[out] = (around[out] + 1) % 3
    X = means[true] + rng.standard_normal((n, D))
    init = (around * 2 + (np.arange(n) // 7) % 2).astype(np.int32)        # every speaker split into two initial clusters
    return X, Phi, init, true, around, out


def test_the_loop_probability_keeps_single_frames_with_their_neighbours():
    X, Phi, init, true, around, out = planted()
    said = {}
    for loop_prob in (0.0, 0.99):
        r = HR.vbx_hmm(X, Phi, init, 6, loop_prob)
        lab = r["gamma"].argmax(1)
        rest = np.setdiff1d(np.arange(len(true)), out)
        spk = np.full(6, -1)
        for s in np.unique(lab[rest]):
            spk[s] = np.bincount(true[rest][lab[rest] == s], minlength=3).argmax()
        said[loop_prob] = spk[lab]
        assert np.array_equal(said[loop_prob][rest], true[rest])         # the runs themselves are found either way
    assert np.array_equal(said[0.99][out], around[out])                  # with the chain: the speaker of the frames around it
    assert np.array_equal(said[0.0][out], true[out])                     # without: the frame's own speaker


def test_the_log_domain_holds_where_probabilities_underflow():
    m, X, init, true = case(7, 2049, 192, 64, 7, 3)
    seen = {}

    def spy(logp, pi, loop_prob, dtype, reverse, fn):
        seen["worst"] = min(seen.get("worst", 0.0), float(logp.max(1).sum()))
        return HR.forward_backward(logp, pi, loop_prob, dtype, reverse, fn)
    r = HR.vbx_hmm(X, m.Phi, init, 7, 0.99, Fa=1.0, max_iters=3, fb=spy)
    print(f"sum_t max_s logp = {seen['worst']:.1f}, elbo {r['elbo'].tolist()}")
    assert seen["worst"] < -2000.0 and np.exp(seen["worst"]) == 0.0      # the likelihood of the sequence is below every float64
    assert np.isfinite(r["elbo"]).all() and np.isfinite(r["gamma"]).all() and np.isfinite(r["lf"]).all() and np.isfinite(r["lb"]).all()
    # a row's gammas sum to 1 up to what lf + lb - tll carries: each of the n steps rounds a number of tll's size once
    assert np.abs(r["gamma"].sum(1) - 1.0).max() <= 2049 * np.spacing(abs(seen["worst"])) and abs(r["pi"].sum() - 1.0) <= 1e-14
    lab = r["gamma"].argmax(1)
    assert all(len(set(true[lab == s])) == 1 for s in np.unique(lab))


def test_a_speaker_with_no_weight_keeps_gamma_zero_and_p_zero_is_exact():
    rng = np.random.default_rng(0)
    logp = rng.standard_normal((20, 4)) * 3
    pi = np.array([0.5, 0.0, 0.3, 0.2])
    for loop_prob in (0.0, 0.9):
        r = HR.forward_backward(logp, pi, loop_prob)
        assert not r["gamma"][:, 1].any() and r["pinew"][1] == 0.0 and np.isfinite(r["gamma"]).all() and np.isfinite(r["tll"])
    r = HR.forward_backward(logp, pi, 0.0)
    with np.errstate(divide="ignore"):
        assert np.array_equal(r["lf"][1:], logp[1:] + (np.log(pi)[None, :] + r["m"][:-1, None]))      # the logaddexp returned its other argument
    assert np.array_equal(HR._logaddexp(np.array([-np.inf, 1.5, -np.inf]), np.array([2.5, -np.inf, -np.inf]), HR._Fn(np.float64)),
                          np.array([2.5, 1.5, -np.inf]))


def test_the_new_symbols_keywords_and_refusals():
    lib = LIB.load_library()
    for name in ("sdk_vbx_hmm_workspace_bytes", "sdk_vbx_hmm"):
        assert hasattr(lib, name) and name in LIB.SIGNATURES
    assert lib.sdk_abi_version() == LIB.ABI_VERSION == 4                  # symbols are only added
    n, D, S = 2049, 128, 130
    assert lib.sdk_vbx_hmm_workspace_bytes(n, D, S) >= lib.sdk_vbx_workspace_bytes(n, D, S) + 8 * (3 * n * S + n)
    assert lib.sdk_vbx_hmm_workspace_bytes(n, 96, S) == 0 and b"D=96" in lib.sdk_last_error()
    assert lib.sdk_vbx_hmm_workspace_bytes(0, D, S) == 0 and lib.sdk_vbx_hmm_workspace_bytes(n, D, 65537) == 0
    # a bad loop_prob is refused before anything else is looked at (no context, no pointers: nothing can have been launched)
    for bad in (float("nan"), -0.1, 1.0, 1.5):
        assert lib.sdk_vbx_hmm(None, None, None, None, 4, 64, 2, 0.07, 0.8, 20, 1e-4, 7.0, bad, None, None, None, None, None, None, 0, None) != 0
        assert b"loop_prob" in lib.sdk_last_error()
    cl, be = sub("cluster"), sub("backend")
    assert cl.VBX_LOOP_PROB == 0.99
    sig = inspect.signature(cl.vbx_cluster)
    assert list(sig.parameters)[-1] == "loop_prob" and sig.parameters["loop_prob"].default == 0.0
    sig = inspect.signature(be.Backend.cluster_ranges)
    assert list(sig.parameters)[-3:] == ["clustering", "loop_prob", "plda"]
    assert (sig.parameters["clustering"].default, sig.parameters["loop_prob"].default, sig.parameters["plda"].default) == ("ahc", cl.VBX_LOOP_PROB, None)
    with pytest.raises(ValueError, match="loop_prob=1.0"):
        cl.vbx_cluster(None, np.zeros((4, 64), np.float32), None, loop_prob=1.0, rows=None)
