"""What tests/test_laplacian_gpu.py relies on, checked without a GPU: the float64 restatement of the Ritz kernel is right (against
numpy.linalg.eigh on every Ritz-step case), every driver case is far from the library's not-SPD rule, the converged case has the gap
it is named for, and the bf16 rounding of the mat-vec alone - measured with tests/laplacian_ref.rounded_S - uses at most half of the
2e-3 the GPU file allows.  Every figure is printed (pytest -s)."""
import numpy as np
import pytest

import laplacian_ref as lr


@pytest.mark.parametrize("kind,k", lr.RITZ_CASES)
def test_jacobi_restated_matches_eigh(kind, k):
    """Eigenvalues and the residual |Q^T H Q - diag(lam)| relative to |H|_2: at most 8.1e-15 measured (k up to 32, repeated eigenvalues
    included), asserted <= 1e-12 - the figure the GPU file adds to its fp32 bounds.  At most 10 sweeps ran: the 30-sweep cap never ends
    the loop."""
    G = lr.ritz_case(kind, k)
    assert G.dtype == np.float32 and G.shape == (k, k)
    H = lr.sym64(G)
    Q, lam, sweeps = lr.jacobi_restated(G)
    Q64, lam64 = lr.eigh_desc(H)
    scale = lr.norm2(H) or 1.0
    e_lam = float(np.abs(lam - lam64).max()) / scale
    e_res = float(np.abs(Q.T @ H @ Q - np.diag(lam)).max()) / scale
    e_orth = float(np.abs(Q.T @ Q - np.eye(k)).max())
    print(f"laplacian_cpu ritz {kind} k={k}: sweeps {sweeps}, |lam - lam64| / |H| = {e_lam:.2e}, residual / |H| = {e_res:.2e}, |Q^T Q - I| = {e_orth:.2e}")
    assert sweeps < 30
    assert e_lam <= 1e-12 and e_res <= 1e-12 and e_orth <= 1e-12
    assert np.all(np.diff(lam) <= 0)
    big = np.abs(Q).argmax(0)
    assert (Q[big, np.arange(k)] > 0).all()
    if kind == "spectrum" and k > 1:                        # built so that every column can be compared one by one
        assert (-np.diff(lam64)).min() >= 1e-3
        assert np.abs(Q - Q64).max() <= 1e-12 / (-np.diff(lam64)).min()
    if kind == "asym" and k > 1:
        assert G[0, k - 1] != G[k - 1, 0]
    if kind == "zero":
        assert sweeps == 0 and not lam.any() and np.array_equal(Q, np.eye(k))


def test_jacobi_restated_contract_on_diagonal_matrices():
    """Distinct permuted entries: the sorted entries and the exact permutation matrix; ties: ascending original index (a selection sort that
    compares values alone gives 3, 2b, 2a for [2a, 2b, 3])."""
    d = np.array([2.0, 2.0, 3.0, 1.0, 3.0, 2.0], dtype=np.float32)
    Q, lam, sweeps = lr.jacobi_restated(np.diag(d))
    assert sweeps == 0 and lam.tolist() == [3, 3, 2, 2, 2, 1]
    assert np.array_equal(Q.argmax(0), [2, 4, 0, 1, 5, 3]) and np.array_equal(np.sort(Q, 0)[:-1], np.zeros((5, 6)))


def _driver_case(N, k, n_iter, E):
    Ef = lr.host_bf16_rows(E)
    V0 = lr.start_block(N, k)
    S = lr.dense_S(Ef)
    exact = lr.driver_ref(Ef, V0, n_iter, S)
    model = lr.driver_ref(Ef, V0, n_iter, lr.rounded_S(Ef))
    dlam = float(np.abs(exact.lam - model.lam).max())
    spread = lr.projector_diff(exact.U, model.U)
    defect = lr.ritz_defect(model.U, model.lam, S)
    print(f"laplacian_cpu driver N={N} k={k} n_iter={n_iter}: least pivot ratio {exact.min_pivot:.3g} (rounded {model.min_pivot:.3g}), "
          f"|lam - lam'| = {dlam:.3g}, |UU^T - U'U'^T|max = {spread:.4g}, max|U'^T S U' - diag(lam')| = {defect:.3g}, lam[0] = {exact.lam[0]:.6f}")
    assert exact.min_pivot >= 1e-4 and model.min_pivot >= 1e-4, "100 x the library's 1e-6 rule: the not-SPD flag cannot legitimately be set"
    assert defect <= 1e-3, "bf16 rounding alone must leave half of the GPU file's 2e-3"
    assert dlam <= 1e-3
    assert np.abs(exact.U.T @ exact.U - np.eye(k)).max() <= 1e-12 and lr.ritz_defect(exact.U, exact.lam, S) <= 1e-12
    return exact, S, spread


@pytest.mark.parametrize("N,k", lr.DRIVER_SHAPES)
@pytest.mark.parametrize("n_iter", lr.DRIVER_ITERS)
def test_driver_cases_are_well_posed_and_rounding_uses_half_the_budget(N, k, n_iter):
    exact, S, spread = _driver_case(N, k, n_iter, lr.driver_rows(N, k))
    table = lr.spread_of(N, k, n_iter)
    assert spread <= table + 1e-14 and table <= 1.1 * spread + 1e-14, "laplacian_ref.SPREAD must hold the measured figure"
    if n_iter == 0:                                         # S plays no part in the span
        Q0 = np.linalg.qr(lr.start_block(N, k).astype(np.float64))[0]
        assert lr.projector_diff(exact.U, Q0) <= 1e-13


def test_converged_case_has_its_gap():
    c = lr.CONVERGED
    exact, S, spread = _driver_case(c["N"], c["k"], c["n_iter"], lr.converged_rows())
    Q, lam = lr.eigh_desc(S)
    k = c["k"]
    gap = float(lam[k - 1] - lam[k])
    print(f"laplacian_cpu converged: lam[:6] = {lam[:6].round(6).tolist()}, gap = {gap:.4f}, driver_ref vs eigh: |lam| {np.abs(exact.lam - lam[:k]).max():.2e}, "
          f"projector {lr.projector_diff(exact.U, Q[:, :k]):.2e}")
    assert gap >= 0.3
    assert np.abs(exact.lam - lam[:k]).max() <= 1e-9 and lr.projector_diff(exact.U, Q[:, :k]) <= 1e-9      # 12 iterations have converged
    assert spread <= lr.SPREAD_CONVERGED and lr.SPREAD_CONVERGED <= 1.1 * spread


def test_rounding_of_A_alone():
    """|S - S_rounded|_2 with only A's entries rounded to bf16 (degrees from the rounded entries), random unit rows."""
    for N in (33, 257, 513):
        Ef = lr.host_bf16_rows(lr.unit_rows(N, 7 + N))
        R = lr.rounded_S(Ef)
        Sr = R.A * R.dinv[:, None] * R.dinv[None, :]
        d = lr.norm2(lr.dense_S(Ef) - Sr)
        print(f"laplacian_cpu |S - S_rounded|_2 at N = {N}: {d:.3g}")
        assert d <= 1e-3


def test_bf16_round_is_torch_s():
    import torch
    x = np.random.default_rng(3).standard_normal(4096).astype(np.float32)
    x[:4] = [1.00390625, 1.01171875, 0.0, -1.00390625]      # ties: to even
    assert np.array_equal(lr.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).double().numpy())
