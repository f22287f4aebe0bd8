"""TEST INFRASTRUCTURE: float64 references of the C spectral driver (sdk_laplacian_topk, Engine.laplacian_topk) and of its device Ritz step
(sdk_sym_eigh, Engine.sym_eigh), in plain numpy and written from the definitions:
  jacobi_restated   the Ritz kernel's loop in float64: same sweep order, same skip of apq == 0, same stop rule, same sort, same sign rule
  dense_S           S = D^-1/2 A D^-1/2, A = max(E E^T, 0), on the bf16 rows taken as float64
  driver_ref        QR of the start block, n_iter x QR(S V), H = V^T S V, eigh, U = V Q - what the driver computes in exact arithmetic
  rounded_S         a host model of the mat-vec kernel's rounding (A and the degrees from bf16-rounded A, X split into bf16 hi + lo), so the
                    CPU file can measure how far that rounding alone moves the answers
plus the case tables, seeds and generators that tests/test_laplacian_cpu.py and tests/test_laplacian_gpu.py share.  Never imported by the
product."""
import math
from collections import namedtuple

import numpy as np

U24 = 2.0 ** -24          # unit roundoff of fp32
KV = 32                   # the widest block the thin kernels and the Ritz step take
D = 192                   # the embedding width the mat-vec kernel is built for


# ------------------------------------------------------------------ the Ritz step
def sign_rule(Q):
    """Each column scaled by +-1 so that its largest-magnitude component (the first of equals) is positive."""
    Q = np.array(Q, dtype=np.float64)
    for c in range(Q.shape[1]):
        big = 0
        for r in range(1, Q.shape[0]):
            if abs(Q[r, c]) > abs(Q[big, c]):
                big = r
        if Q[big, c] < 0:
            Q[:, c] = -Q[:, c]
    return Q


def jacobi_restated(G):
    """-> (Q [k, k], lam [k], sweeps): the kernel's cyclic Jacobi on H = (G + G^T) / 2 in float64.  Rotations over (p, q), p < q, in row
    order; a pair with apq == 0 is skipped; a sweep starts only while off^2 > 1e-30 (diag^2 + 1e-300), at most 30 sweeps.  Eigenvalues
    descending, equal ones in ascending order of their diagonal position; columns of Q by sign_rule.  sweeps = the sweeps that ran."""
    G = np.asarray(G, dtype=np.float64)
    k = G.shape[0]
    A = 0.5 * (G + G.T)
    V = np.eye(k)
    sweeps = 0
    for _ in range(30):
        off = diag = 0.0
        for i in range(k):
            diag += A[i, i] * A[i, i]
            for j in range(i + 1, k):
                off += A[i, j] * A[i, j]
        if off <= 1e-30 * (diag + 1e-300):
            break
        sweeps += 1
        for p in range(k - 1):
            for q in range(p + 1, k):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                ap, aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
                ap, aq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * ap - s * aq, s * ap + c * aq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    order = list(range(k))
    for i in range(k):                                    # the kernel's selection sort: descending, ties -> lower index first
        for j in range(i + 1, k):
            aj, ai = A[order[j], order[j]], A[order[i], order[i]]
            if aj > ai or (aj == ai and order[j] < order[i]):
                order[i], order[j] = order[j], order[i]
    lam = np.array([A[o, o] for o in order])
    return sign_rule(V[:, order]), lam, sweeps


def eigh_desc(H):
    """numpy's eigh, eigenvalues descending, columns by sign_rule."""
    w, Q = np.linalg.eigh(np.asarray(H, dtype=np.float64))
    return sign_rule(Q[:, ::-1]), w[::-1].copy()


def sym64(G):
    G = np.asarray(G, dtype=np.float64)
    return 0.5 * (G + G.T)


def norm2(H):
    return float(np.linalg.norm(H, 2)) if H.size else 0.0


def clusters(lam64, tol=1e-3):
    """Runs of a descending eigenvalue list whose neighbours are closer than tol -> [(first, last + 1), ...]."""
    out, a = [], 0
    for i in range(1, len(lam64) + 1):
        if i == len(lam64) or lam64[i - 1] - lam64[i] >= tol:
            out.append((a, i))
            a = i
    return out


# ------------------------------------------------------------------ the driver
def bf16_round(x):
    """float64 / float32 -> the nearest bf16 (ties to even), returned as float64."""
    b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def affinity(Ef):
    Ef = np.asarray(Ef, dtype=np.float64)
    return np.maximum(Ef @ Ef.T, 0.0)


def dense_S(Ef):
    """S = D^-1/2 A D^-1/2 with A = max(E E^T, 0) and D = diag(A 1), in float64 on the rows as given."""
    A = affinity(Ef)
    dinv = 1.0 / np.sqrt(A.sum(1))
    return A * dinv[:, None] * dinv[None, :]


class rounded_S:
    """The operator the device applies, as far as its number formats go: A's entries rounded to bf16 (the kernel rounds each tile of
    max(E E^T, 0) in registers), the degrees summed from THOSE entries, D^-1/2 in fp32, and the operand x = D^-1/2 V, held in fp32, split
    into bf16 hi + bf16 lo (pack_x_kernel: hi = bf16(x), lo = bf16(x - hi)).  Sums are float64: the order of the fp32 accumulation is not
    modelled (it is three orders of magnitude below the bf16 rounding of A)."""

    def __init__(self, Ef):
        self.A = bf16_round(affinity(Ef))
        self.dinv = (1.0 / np.sqrt(self.A.sum(1))).astype(np.float32).astype(np.float64)

    def __matmul__(self, V):
        x = (self.dinv[:, None] * np.asarray(V, dtype=np.float64)).astype(np.float32).astype(np.float64)
        hi = bf16_round(x)
        x = hi + bf16_round(x - hi)
        return (self.A @ x).astype(np.float32).astype(np.float64) * self.dinv[:, None]


DriverRef = namedtuple("DriverRef", "U lam V min_pivot")


def qr_pos(Y):
    """-> (Q, least pivot ratio): the QR factor with R's diagonal positive - what CholeskyQR2 computes in exact arithmetic - and
    min_j L_jj^2 / G_jj for G = Y^T Y = L L^T (L = R^T), the quantity sdk_chol_inverse's relative-pivot rule looks at."""
    Q, R = np.linalg.qr(Y)
    d = np.diag(R)
    s = np.where(d < 0, -1.0, 1.0)
    ratio = float((d * d / (Y * Y).sum(0)).min())
    return Q * s[None, :], ratio


def driver_ref(Ef, V0, n_iter, S=None):
    """The driver in float64: V = qr(V0); n_iter x V = qr(S V); H = V^T S V symmetrised; eigh descending; U = V Q.  S: dense_S(Ef) by
    default, or anything with S @ V (a matrix, or rounded_S).  min_pivot is the least pivot ratio over every block that was
    orthogonalised (the second pass of CholeskyQR2 sees a Gram matrix within rounding of I: ratio 1)."""
    S = dense_S(Ef) if S is None else S
    V, piv = qr_pos(np.asarray(V0, dtype=np.float64))
    for _ in range(n_iter):
        V, p = qr_pos(S @ V)
        piv = min(piv, p)
    H = V.T @ (S @ V)
    Q, lam = eigh_desc(0.5 * (H + H.T))
    return DriverRef(V @ Q, lam, V, piv)


def projector_diff(U, W):
    U, W = np.asarray(U, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return float(np.abs(U @ U.T - W @ W.T).max())


def ritz_defect(U, lam, S64):
    """max |U^T S U - diag(lam)| against the exact operator."""
    U = np.asarray(U, dtype=np.float64)
    return float(np.abs(U.T @ S64 @ U - np.diag(np.asarray(lam, dtype=np.float64))).max())


# ------------------------------------------------------------------ shared cases and generators
RITZ_K = (1, 2, 7, 16, 31, 32)
RITZ_KINDS = ("gaussian", "spectrum", "triples", "negdef", "neardiag", "asym", "zero")


def case_seed(*shape):
    s = 31337
    for v in shape:
        s = s * 1009 + int(v)
    return s


def _orth(k, rng):
    return np.linalg.qr(rng.standard_normal((k, k)))[0]


def ritz_case(kind, k):
    """-> G fp32 [k, k] (what the device is given; the reference takes it to float64 and symmetrises)."""
    rng = np.random.default_rng(case_seed(k, RITZ_KINDS.index(kind)))
    if kind == "gaussian" or kind == "asym":
        M = rng.standard_normal((k, k))
        G = (M + M.T).astype(np.float32)
        if kind == "asym":
            G[0, k - 1] += np.float32(1e-3)                 # k = 1: the one entry; else G != G^T and the kernel must symmetrise
        return G
    if kind == "spectrum":
        Q = _orth(k, rng)
        return (Q @ np.diag(np.linspace(1.0, 0.05, k)) @ Q.T).astype(np.float32)
    if kind == "triples":
        Q = _orth(k, rng)
        return (Q @ np.diag(1.0 - 0.08 * (np.arange(k) // 3)) @ Q.T).astype(np.float32)
    if kind == "negdef":
        M = rng.standard_normal((k, k))
        return (-(M @ M.T)).astype(np.float32)
    if kind == "neardiag":
        M = rng.standard_normal((k, k))
        return (np.diag(rng.permutation(np.linspace(1.0, 2.0, k))) + 1e-9 * (M + M.T)).astype(np.float32)
    if kind == "zero":
        return np.zeros((k, k), dtype=np.float32)
    raise KeyError(kind)


RITZ_CASES = [(kind, k) for k in RITZ_K for kind in RITZ_KINDS]

# (N, k): N = k, N below one 32-row tile / one 256-row block, one past a tile / a block, two blocks and a row, k = 1 and k = 32
DRIVER_SHAPES = [(1, 1), (2, 2), (32, 32), (33, 7), (255, 31), (256, 16), (257, 32), (513, 2), (700, 1)]
DRIVER_ITERS = (0, 1, 12)
CONVERGED = dict(N=513, k=4, n_iter=12, clusters=4, noise=0.3, seed=11)

# The rounding spread of every driver case with n_iter >= 1: |U U^T - U' U'^T|max between driver_ref on dense_S and on rounded_S, as
# tests/test_laplacian_cpu.py measures and prints it (it asserts that the figure here is the measured one, rounded up by at most 10 %).
# The GPU file allows the device SPREAD_FACTOR x this figure plus PROJ_FP32 against driver_ref on dense_S.  The factor is 2, not 4: the
# host model already holds the rounding of the operand X, so nothing the kernel rounds is left out of it; PROJ_FP32 is what the fp32
# steps that have no bf16 in them (CholeskyQR2, U = V Q) are allowed at n_iter = 0, where the spread is zero (as it is for N = k).
SPREAD_FACTOR = 2.0
PROJ_FP32 = 1e-5
SPREAD = {                                   # (N, k): (n_iter = 1, n_iter = 12); measured 3.596e-4 / 7.802e-4, 2.444e-4 / 4.016e-4, ...
    (1, 1): (0.0, 0.0),                      # N = k: U spans everything, both projectors are I
    (2, 2): (0.0, 0.0),
    (32, 32): (0.0, 0.0),
    (33, 7): (3.6e-4, 7.9e-4),
    (255, 31): (2.5e-4, 4.1e-4),
    (256, 16): (2.2e-4, 3.1e-4),
    (257, 32): (3.4e-4, 4.9e-4),
    (513, 2): (3.9e-5, 3.1e-5),
    (700, 1): (2.7e-5, 4.7e-7),
}
SPREAD_CONVERGED = 3.3e-6                    # measured 3.21e-6


def spread_of(N, k, n_iter):
    return 0.0 if n_iter == 0 else SPREAD[(N, k)][0 if n_iter == 1 else 1]


def converged_rows():
    from oracle import spectral as ospec
    c = CONVERGED
    return ospec.vmf_mixture(c["N"], D, c["clusters"], c["seed"], noise=c["noise"])[0]


def start_block(N, k):
    return np.random.default_rng(case_seed(N, k) + 1).standard_normal((N, k)).astype(np.float32)


def unit_rows(N, seed, d=D):
    x = np.random.default_rng(seed).standard_normal((N, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def driver_rows(N, k):
    """fp32 unit gaussian rows of a driver case (the GPU file takes them through Engine.l2norm; host_bf16_rows models that)."""
    return unit_rows(N, case_seed(N, k))


def host_bf16_rows(E):
    """The rows as the kernel sees them, modelled on the host: normalised in float64, rounded to bf16."""
    E = np.asarray(E, dtype=np.float64)
    return bf16_round(E / np.linalg.norm(E, axis=1, keepdims=True))
