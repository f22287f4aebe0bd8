"""The C spectral driver (csrc/collective.hip sdk_laplacian_topk, Engine.laplacian_topk) and its device Ritz step (sdk_sym_eigh,
Engine.sym_eigh: the driver's jacobi_eigh_kernel on its own) against the float64 references of tests/laplacian_ref.py.

Ritz step (u = 2^-24, H = (G + G^T) / 2 in float64, lam64 / Q64 from numpy.linalg.eigh):
  lam descending with no slack
  |lam - lam64|            <= u |lam64| + 1e-12 |H|_2      float64 inside, rounded once; 1e-12 from tests/test_laplacian_cpu.py (8.1e-15 measured)
  |Q^T H Q - diag(lam)|max <= (2k + 2) u |H|_2             each entry of Q carries one fp32 rounding
  |Q^T Q - I|max           <= (k + 2) u
  |q - q64|max             <= u + 1e-12 / gap              per column whose gap to both neighbours is >= 1e-3, q64 by the sign rule
  |P - P64|max             <= 3 u + 2e-12 |H|_2 / gap      per cluster of eigenvalues closer than 1e-3, P = Q_c Q_c^T: an entry is a sum
                                                           of products of two once-rounded factors, 2 u sum_c |q_ic||q_jc| <= 2 u
and the contract bit for bit on diagonal matrices (sort order, ties by index, sign rule, k = 1).

Driver: the rows the kernel sees -> S64 = dense_S, ref = driver_ref; flag 0, finite, |U^T U - I| < 1e-4, lam descending within 1e-7,
lam[0] <= 1 + 2e-3, max|U^T S64 U - diag(lam)| <= 2e-3 (the project's figure for bf16 tile rounding inside A V; rounding alone uses at
most 2.5e-4 of it, tests/test_laplacian_cpu.py), n_iter = 0: projector of qr(V0) within 1e-5; n_iter >= 1: |lam - ref.lam| <= 2e-3 and the
projector within laplacian_ref.SPREAD_FACTOR x the case's rounding spread + PROJ_FP32 of ref.U.  Every figure is printed before it is
asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import laplacian_ref as lr
pytestmark = pytest.mark.gpu

U24 = lr.U24


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def ratio(err, bound):
    """max err / bound over the elements; an exact element counts as 0 whatever its bound (0 / 0 on the zero matrix)."""
    err = np.abs(np.asarray(err, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def eigh_gpu(engine, G):
    Q, lam = engine.sym_eigh(dev(G))
    return host(Q), host(lam)


# ------------------------------------------------------------------ the Ritz step alone
@pytest.mark.parametrize("kind,k", lr.RITZ_CASES)
def test_sym_eigh_against_float64(engine, kind, k):
    G = lr.ritz_case(kind, k)
    Q, lam = eigh_gpu(engine, G)
    assert Q.dtype == np.float32 and lam.dtype == np.float32 and Q.shape == (k, k) and lam.shape == (k,)
    assert np.isfinite(Q).all() and np.isfinite(lam).all()
    H = lr.sym64(G)
    Q64, lam64 = lr.eigh_desc(H)
    nH = lr.norm2(H)
    Qd, ld = Q.astype(np.float64), lam.astype(np.float64)
    r_lam = ratio(ld - lam64, U24 * np.abs(lam64) + 1e-12 * nH)
    r_res = ratio(Qd.T @ H @ Qd - np.diag(ld), (2 * k + 2) * U24 * nH)
    r_orth = ratio(Qd.T @ Qd - np.eye(k), (k + 2) * U24)
    gaps = np.full(k, np.inf)
    if k > 1:
        d = -np.diff(lam64)
        gaps[:-1] = d
        gaps[1:] = np.minimum(gaps[1:], d)
    cols = np.flatnonzero(gaps >= 1e-3)
    r_vec = max([ratio(Qd[:, c] - Q64[:, c], U24 + 1e-12 / gaps[c]) for c in cols], default=0.0)
    r_proj = 0.0
    cl = lr.clusters(lam64)
    for a, b in cl:
        gap = min(lam64[a - 1] - lam64[a] if a > 0 else np.inf, lam64[b - 1] - lam64[b] if b < k else np.inf)
        P, P64 = Qd[:, a:b] @ Qd[:, a:b].T, Q64[:, a:b] @ Q64[:, a:b].T
        r_proj = max(r_proj, ratio(P - P64, 3 * U24 + 2e-12 * nH / gap))
    print(f"laplacian ritz {kind} k={k}: err / bound: lam {r_lam:.3f}, residual {r_res:.3f}, orthonormality {r_orth:.3f}, "
          f"{len(cols)} separated columns {r_vec:.3f}, {len(cl)} cluster projectors {r_proj:.3f}")
    assert np.all(np.diff(lam) <= 0), "lam must be descending with no slack"
    assert r_lam <= 1.0 and r_res <= 1.0 and r_orth <= 1.0
    assert r_vec <= 1.0 and r_proj <= 1.0
    if kind == "spectrum":
        assert len(cols) == k, "built so that every column is compared one by one"
    if kind == "triples" and k >= 3:
        assert max(b - a for a, b in cl) == 3
    big = np.abs(Q).argmax(0)
    assert (Q[big, np.arange(k)] > 0).all(), "the largest-magnitude component of every column must be positive"
    Q2, lam2 = eigh_gpu(engine, G)
    assert np.array_equal(bits(Q2), bits(Q)) and np.array_equal(bits(lam2), bits(lam)), "two runs must be bit-identical"
    if kind == "zero":
        assert not bits(lam).any() and np.array_equal(Q, np.eye(k, dtype=np.float32))


@pytest.mark.parametrize("k", lr.RITZ_K)
def test_sym_eigh_contract_on_diagonal_matrices(engine, k):
    """No rotation runs on a diagonal matrix (every apq is 0), so the answer is the sort and the sign rule alone, bit for bit."""
    rng = np.random.default_rng(lr.case_seed(k, 99))
    d = rng.permutation(np.linspace(-1.0, 2.0, k)).astype(np.float32) if k > 1 else np.array([-0.75], dtype=np.float32)
    Q, lam = eigh_gpu(engine, np.diag(d))
    order = np.argsort(-d.astype(np.float64), kind="stable")
    assert np.array_equal(bits(lam), bits(d[order])), "lam must be the entries themselves, sorted descending"
    want = np.zeros((k, k), dtype=np.float32)
    want[order, np.arange(k)] = 1.0
    assert np.array_equal(bits(Q), bits(want)), "Q must be the exact 0 / 1 permutation matrix (+0.0 and +1.0)"
    # ties: each value three (or fewer) times, scattered; the tied columns come in ascending original index
    t = rng.permutation(np.repeat(np.arange((k + 2) // 3, dtype=np.float32), 3)[:k])
    Q, lam = eigh_gpu(engine, np.diag(t))
    order = np.argsort(-t.astype(np.float64), kind="stable")                           # stable: equal entries keep ascending index
    want = np.zeros((k, k), dtype=np.float32)
    want[order, np.arange(k)] = 1.0
    assert np.array_equal(bits(lam), bits(t[order]))
    assert np.array_equal(bits(Q), bits(want)), f"ties must go to the lower index first: got columns {Q.argmax(0).tolist()}, want {order.tolist()}"
    if k >= 3:                                                                         # the order a value-only selection sort gets wrong
        Q, lam = eigh_gpu(engine, np.diag(np.array([2, 2, 3] + [0] * (k - 3), dtype=np.float32)))
        assert Q.argmax(0)[:3].tolist() == [2, 0, 1] and lam[:3].tolist() == [3, 2, 2]
    # a negative largest component is flipped: G = [[0, -1], [-1, 0]] embedded; eigenvectors (1, -1) / sqrt 2 and (1, 1) / sqrt 2
    if k >= 2:
        G = np.zeros((k, k), dtype=np.float32)
        G[0, 1] = G[1, 0] = -1.0
        G[np.arange(2, k), np.arange(2, k)] = -5.0
        Q, lam = eigh_gpu(engine, G)
        assert lam[0] == 1.0 and lam[1] == -1.0
        assert Q[0, 0] > 0 and Q[1, 0] < 0 and Q[0, 1] > 0 and Q[1, 1] > 0, "first of two equal magnitudes decides the sign"
        assert np.abs(np.abs(Q[:2, :2]) - np.sqrt(0.5)).max() <= U24


def test_sym_eigh_k1(engine):
    for v in (3.5, -2.25, 0.0):
        Q, lam = eigh_gpu(engine, np.array([[v]], dtype=np.float32))
        assert Q.tolist() == [[1.0]] and lam.tolist() == [v]


def test_sym_eigh_refusals(engine):
    lib = engine.lib
    G = dev(lr.ritz_case("gaussian", 7))
    want = [host(t).copy() for t in engine.sym_eigh(G)]
    big = torch.zeros((33, 33), dtype=torch.float32, device="cuda")
    Q, lam = torch.empty_like(big), torch.empty(33, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def still_works():
        got = [host(t) for t in engine.sym_eigh(G)]
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))

    for k in (0, 33, -1):
        assert lib.sdk_sym_eigh(engine.ctx, big.data_ptr(), k, Q.data_ptr(), lam.data_ptr(), stream) != 0
        assert f"k={k}".encode() in lib.sdk_last_error() and b"sdk_sym_eigh" in lib.sdk_last_error()
        still_works()
    for args in ((None, 7, Q.data_ptr(), lam.data_ptr()), (big.data_ptr(), 7, None, lam.data_ptr()), (big.data_ptr(), 7, Q.data_ptr(), None)):
        assert lib.sdk_sym_eigh(engine.ctx, *args, stream) != 0 and b"sdk_sym_eigh: null argument" in lib.sdk_last_error()
    still_works()
    wide = torch.zeros((7, 14), dtype=torch.float32, device="cuda")
    for call in (lambda: engine.sym_eigh(G.double()), lambda: engine.sym_eigh(G[:, :6]), lambda: engine.sym_eigh(G.cpu()), lambda: engine.sym_eigh(big),
                 lambda: engine.sym_eigh(wide[:, ::2]), lambda: engine.sym_eigh(G[0]), lambda: engine.sym_eigh(torch.zeros((0, 0), device="cuda"))):
        with pytest.raises(ValueError, match=r"sym_eigh: .*\b(G|k)\b"):
            call()
        still_works()


# ------------------------------------------------------------------ the driver
_CACHE = {}


def driver_case(engine, N, k, rows=None):
    """Rows through Engine.l2norm (computed once per shape and shared), what the kernel sees as float64, S64, the start block."""
    key = (N, k) if rows is None else "converged"
    if key not in _CACHE:
        E = lr.driver_rows(N, k) if rows is None else rows
        _, Eb, _ = engine.l2norm(dev(E))
        Ef = host(Eb.float()).astype(np.float64)
        _CACHE[key] = (Eb, Ef, lr.dense_S(Ef), lr.start_block(N, k))
    return _CACHE[key]


def run_driver(engine, Eb, V0, n_iter):
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    Vd = dev(V0)
    U, lam = engine.laplacian_topk(Eb, Vd, n_iter, flag=flag)
    U, lam = host(U), host(lam)
    assert np.array_equal(bits(host(Vd)), bits(V0)), "V0 must be unchanged after the call"
    return U, lam, int(flag.item())


def check_common(what, U, lam, flag, S64, k):
    Ud, ld = U.astype(np.float64), lam.astype(np.float64)
    finite = bool(np.isfinite(U).all() and np.isfinite(lam).all())
    orth = float(np.abs(Ud.T @ Ud - np.eye(k)).max())
    desc = float(np.diff(lam).max()) if k > 1 else 0.0
    defect = lr.ritz_defect(Ud, ld, S64)
    print(f"laplacian driver {what}: flag {flag}, finite {finite}, |U^T U - I| = {orth:.3g}, max lam step {desc:.3g}, lam[0] = {lam[0]:.7f}, "
          f"max|U^T S64 U - diag(lam)| = {defect:.3g} (/ 2e-3 = {defect / 2e-3:.3f})")
    assert flag == 0 and finite
    assert orth < 1e-4
    assert desc <= 1e-7
    assert lam[0] <= 1 + 2e-3
    assert defect <= 2e-3


@pytest.mark.parametrize("N,k", lr.DRIVER_SHAPES)
@pytest.mark.parametrize("n_iter", lr.DRIVER_ITERS)
def test_driver_against_float64(engine, N, k, n_iter):
    Eb, Ef, S64, V0 = driver_case(engine, N, k)
    U, lam, flag = run_driver(engine, Eb, V0, n_iter)
    assert U.shape == (N, k) and lam.shape == (k,)
    check_common(f"N={N} k={k} n_iter={n_iter}", U, lam, flag, S64, k)
    ref = lr.driver_ref(Ef, V0, n_iter, S64)
    dlam = float(np.abs(lam - ref.lam).max())
    proj = lr.projector_diff(U, ref.U)
    if n_iter == 0:
        p0 = lr.projector_diff(U, np.linalg.qr(V0.astype(np.float64))[0])
        print(f"laplacian driver N={N} k={k} n_iter=0: projector against qr(V0) {p0:.3g} (/ 1e-5 = {p0 / 1e-5:.3f}), |lam - ref.lam| = {dlam:.3g}")
        assert p0 <= 1e-5, "with no iteration U spans exactly the columns of V0"
    else:
        bound = lr.SPREAD_FACTOR * lr.spread_of(N, k, n_iter) + lr.PROJ_FP32
        print(f"laplacian driver N={N} k={k} n_iter={n_iter}: |lam - ref.lam| = {dlam:.3g} (/ 2e-3 = {dlam / 2e-3:.3f}), projector against ref.U {proj:.4g} "
              f"(/ bound {bound:.3g} = {proj / bound:.3f}; the rounding spread of the case is {lr.spread_of(N, k, n_iter):.3g})")
        assert dlam <= 2e-3
        assert proj <= bound
    U2, lam2, _ = run_driver(engine, Eb, V0, n_iter)
    assert np.array_equal(bits(U2), bits(U)) and np.array_equal(bits(lam2), bits(lam)), "two runs from the same V0 must be bit-identical"


def test_driver_converged_case(engine):
    c = lr.CONVERGED
    N, k = c["N"], c["k"]
    Eb, Ef, S64, V0 = driver_case(engine, N, k, rows=lr.converged_rows())
    U, lam, flag = run_driver(engine, Eb, V0, c["n_iter"])
    check_common("converged", U, lam, flag, S64, k)
    Q64, lam64 = lr.eigh_desc(S64)
    ref = lr.driver_ref(Ef, V0, c["n_iter"], S64)
    dlam = float(np.abs(lam - lam64[:k]).max())
    proj, proj_e = lr.projector_diff(U, ref.U), lr.projector_diff(U, Q64[:, :k])
    bound = lr.SPREAD_FACTOR * lr.SPREAD_CONVERGED + lr.PROJ_FP32
    print(f"laplacian driver converged: gap {lam64[k - 1] - lam64[k]:.4f}, |lam - eigh(S64)| = {dlam:.3g} (/ 2e-3 = {dlam / 2e-3:.4f}), top-{k} projector against "
          f"ref.U {proj:.3g}, against eigh(S64) {proj_e:.3g} (/ bound {bound:.3g} = {max(proj, proj_e) / bound:.3f})")
    assert lam64[k - 1] - lam64[k] >= 0.3
    assert dlam <= 2e-3
    assert proj <= bound and proj_e <= bound
    U2, lam2, _ = run_driver(engine, Eb, V0, c["n_iter"])
    assert np.array_equal(bits(U2), bits(U)) and np.array_equal(bits(lam2), bits(lam))


def test_driver_rank_loss_sets_the_flag_and_nothing_else(engine):
    """k above the rank: ordinary arithmetic (a pivot under the rule), reported through the sticky flag; nothing is raised and the next
    valid call starts from a fresh flag at 0 and gives its earlier result."""
    Eb, Ef, S64, V0 = driver_case(engine, 33, 7)
    want = run_driver(engine, Eb, V0, 1)
    assert want[2] == 0
    _, Eb3, _ = engine.l2norm(dev(lr.unit_rows(3, 5)))
    dup = np.repeat(lr.unit_rows(3, 6), 20, axis=0)                                      # 60 rows, 3 distinct
    _, Ebd, _ = engine.l2norm(dev(dup))
    for what, E, n, k, n_iter in (("N = 3, k = 6", Eb3, 3, 6, 0), ("N = 3, k = 6", Eb3, 3, 6, 2), ("duplicate rows, k = 6 > 3 distinct", Ebd, 60, 6, 4)):
        _, _, flag = run_driver(engine, E, np.random.default_rng(n + k).standard_normal((n, k)).astype(np.float32), n_iter)
        print(f"laplacian driver rank loss ({what}, n_iter = {n_iter}): flag {flag}")
        assert flag == 1
        got = run_driver(engine, Eb, V0, 1)
        assert got[2] == 0 and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


def test_driver_wrapper_refusals(engine, monkeypatch):
    """Everything the C entry cannot see through its bare pointers is a ValueError naming the argument, before the scratch allocation and
    any launch; the valid call afterwards is bit-identical."""
    N, k = 33, 7
    Eb, Ef, S64, V0h = driver_case(engine, N, k)
    V0 = dev(V0h)
    want = run_driver(engine, Eb, V0h, 1)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    wide = torch.zeros((N, 256), dtype=torch.bfloat16, device="cuda")
    wide[:, :192] = Eb
    Vwide = torch.zeros((N, 2 * k), dtype=torch.float32, device="cuda")
    asked = []
    real = engine._scratch_bytes
    monkeypatch.setattr(engine, "_scratch_bytes", lambda key, nbytes: (asked.append(key), real(key, nbytes))[1])
    refusals = [
        ("Eb_all", lambda: engine.laplacian_topk(wide, V0, 1)),                         # ResNet34-width rows read as [N, 192]
        ("Eb_all", lambda: engine.laplacian_topk(wide[:, :192], V0, 1)),                # right width, not contiguous
        ("Eb_all", lambda: engine.laplacian_topk(Eb[:, :128], V0, 1)),
        ("Eb_all", lambda: engine.laplacian_topk(Eb[0], V0[:1], 1)),
        ("Eb_all", lambda: engine.laplacian_topk(Eb.reshape(N, 2, 96), V0, 1)),
        ("Eb_all", lambda: engine.laplacian_topk(Eb.float(), V0, 1)),
        ("Eb_all", lambda: engine.laplacian_topk(Eb.cpu(), V0, 1)),
        ("V0", lambda: engine.laplacian_topk(Eb, V0.double(), 1)),
        ("V0", lambda: engine.laplacian_topk(Eb, V0[:, 0], 1)),
        ("V0", lambda: engine.laplacian_topk(Eb, V0.cpu(), 1)),
        ("V0", lambda: engine.laplacian_topk(Eb, V0[:-1], 1)),                          # fewer rows than the call owns: read and written past the clone
        ("V0", lambda: engine.laplacian_topk(Eb, torch.zeros((N + 1, k), device="cuda"), 1)),
        ("V0", lambda: engine.laplacian_topk(Eb, V0, 1, row0=0, rows=N - 1)),
        ("V0", lambda: engine.laplacian_topk(Eb, torch.zeros((N, 33), device="cuda"), 1)),
        ("V0", lambda: engine.laplacian_topk(Eb, torch.zeros((N, 0), device="cuda"), 1)),
        ("rows", lambda: engine.laplacian_topk(Eb, V0[:0], 1, rows=0)),
        ("rows", lambda: engine.laplacian_topk(Eb, V0, 1, row0=N)),
        ("row0", lambda: engine.laplacian_topk(Eb, V0, 1, row0=-1, rows=N)),
        ("rows", lambda: engine.laplacian_topk(Eb, V0, 1, row0=1, rows=N)),             # row0 + rows > N
        ("n_iter", lambda: engine.laplacian_topk(Eb, V0, -1)),
        ("flag", lambda: engine.laplacian_topk(Eb, V0, 1, flag=flag.long())),
        ("flag", lambda: engine.laplacian_topk(Eb, V0, 1, flag=flag.cpu())),
        ("flag", lambda: engine.laplacian_topk(Eb, V0, 1, flag=torch.zeros(2, dtype=torch.int32, device="cuda"))),
        ("flag", lambda: engine.laplacian_topk(Eb, V0, 1, flag=0)),
    ]
    for arg, call in refusals:
        asked.clear()
        with pytest.raises(ValueError, match=rf"laplacian_topk: .*\b{arg}\b"):
            call()
        assert not asked, f"the refusal ({arg}) must come before the scratch allocation"
        got = run_driver(engine, Eb, V0h, 1)
        assert "laplacian" in asked
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), f"the valid call after a refusal ({arg}) differs"
    # a column slice of V0 that .contiguous() covers is still taken, and gives the result of its contiguous copy
    Vwide[:, :k] = V0
    U, lam = engine.laplacian_topk(Eb, Vwide[:, :k], 1)
    assert np.array_equal(bits(host(U)), bits(want[0])) and np.array_equal(bits(host(lam)), bits(want[1]))


def test_driver_c_entry_refusals(engine):
    lib = engine.lib
    N, k, n_iter = 33, 7, 1
    Eb, Ef, S64, V0h = driver_case(engine, N, k)
    want = run_driver(engine, Eb, V0h, n_iter)
    need = lib.sdk_laplacian_topk_workspace_bytes(N, k)
    assert need > 0 and lib.sdk_laplacian_topk_workspace_bytes(N, 33) == 0 and lib.sdk_laplacian_topk_workspace_bytes(0, k) == 0
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    lam = torch.empty(33, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(V, kk=k, rows=N, ws_ptr=ws.data_ptr(), ws_bytes=need, it=n_iter):
        return lib.sdk_laplacian_topk(engine.ctx, Eb.data_ptr(), N, 0, rows, kk, it, V, lam.data_ptr(), None, ws_ptr, ws_bytes, None, 1, stream)

    V = dev(V0h).clone()
    assert call(V.data_ptr()) == 0                                                       # the bare entry on an exactly sized workspace
    assert np.array_equal(bits(host(V)), bits(want[0])) and np.array_equal(bits(host(lam)[:k]), bits(want[1]))
    V33 = torch.zeros((N, 33), dtype=torch.float32, device="cuda")
    cases = [
        (f"workspace of {need - 1} bytes, {need} needed (sdk_laplacian_topk_workspace_bytes)", lambda: call(V.data_ptr(), ws_bytes=need - 1)),
        ("must be 256-byte aligned", lambda: call(V.data_ptr(), ws_ptr=ws.data_ptr() + 16, ws_bytes=need + 256)),
        ("bad shape", lambda: call(V33.data_ptr(), kk=33, ws_bytes=need + 512)),
        ("bad shape", lambda: call(V.data_ptr(), kk=0)),
        ("bad shape", lambda: call(V.data_ptr(), it=-1)),
        ("without a communicator the call owns all N rows", lambda: call(V.data_ptr(), rows=N - 1)),
        ("null argument", lambda: call(None)),
    ]
    for msg, f in cases:
        before = host(V).copy()
        assert f() != 0, msg
        err = lib.sdk_last_error().decode()
        assert "sdk_laplacian_topk" in err and msg in err, err
        assert np.array_equal(bits(host(V)), bits(before)), "a refused call must not touch V"
        got = run_driver(engine, Eb, V0h, n_iter)
        assert got[2] == 0 and np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), f"after the refusal '{msg}'"
