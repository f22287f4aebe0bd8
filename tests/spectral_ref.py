"""TEST INFRASTRUCTURE: float64 references of the thin [n, k] device primitives of spectral clustering (Engine.rows_gram, rows_apply,
rows_unit, kmeans_assign, kmeans_mindist, chol_inverse), written from each operation's definition as plain loops over rows, centres and
matrix entries, plus the one fp32 restatement the tests need (the per-block partial sums of kmeans_assign, whose order is part of its
contract).  Also the shapes, seeds and generators that tests/test_spectral_primitives_cpu.py and tests/test_spectral_primitives_gpu.py
share, so the CPU file can check the conditions the GPU file relies on.  Never imported by the product."""
import math

import numpy as np

U24 = 2.0 ** -24          # unit roundoff of fp32
BLOCK = 256               # rows per block of kmeans_assign's partial sums (and of rows_gram's first stage)


# ------------------------------------------------------------------ references (float64)
def gram(X, Y):
    """G[a, b] = sum_r X[r, a] Y[r, b], rows added in ascending order."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n, k = X.shape
    G = np.zeros((k, k))
    for r in range(n):
        for a in range(k):
            G[a, :] += X[r, a] * Y[r, :]
    return G


def apply(X, R, scale=None):
    """Y[i, c] = scale[i] * sum_a X[i, a] R[a, c]  (scale None = 1)."""
    X = np.asarray(X, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    n, k = X.shape
    Y = np.zeros((n, k))
    for i in range(n):
        for a in range(k):
            Y[i, :] += X[i, a] * R[a, :]
        if scale is not None:
            Y[i, :] *= float(scale[i])
    return Y


def unit(X):
    """Rows divided by max(their Euclidean norm, 1e-12)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.zeros_like(X)
    for i in range(X.shape[0]):
        ss = 0.0
        for c in range(X.shape[1]):
            ss += X[i, c] * X[i, c]
        Y[i, :] = X[i, :] / max(math.sqrt(ss), 1e-12)
    return Y


def _dist2(x, c):
    """x, c: lists of Python floats (float64)."""
    d = 0.0
    for j in range(len(x)):
        t = x[j] - c[j]
        d += t * t
    return d


def assign(R, C):
    """-> (label int32 [n], dist2 [n], margin [n]): the nearest centre with ties to the lowest index, the squared distance to it, and
    second-best minus best (inf with one centre).  A row whose every distance is NaN gets label -1, dist2 inf, margin NaN."""
    R = np.asarray(R, dtype=np.float64).tolist()
    C = np.asarray(C, dtype=np.float64).tolist()
    n = len(R)
    lab = np.full(n, -1, dtype=np.int32)
    d2 = np.full(n, np.inf)
    margin = np.full(n, np.nan)
    for i in range(n):
        best, bd, sd = -1, math.inf, math.inf
        for q in range(len(C)):
            d = _dist2(R[i], C[q])
            if d < bd:
                best, bd, sd = q, d, bd
            elif d < sd:
                sd = d
        lab[i], d2[i] = best, bd
        if best >= 0:
            margin[i] = sd - bd
    return lab, d2, margin


def mindist(R, c, d2, first):
    """d2'[i] = |R[i] - c|^2 when first, else min(d2[i], |R[i] - c|^2)."""
    R = np.asarray(R, dtype=np.float64).tolist()
    c = np.asarray(c, dtype=np.float64).tolist()
    out = np.zeros(len(R))
    for i in range(len(R)):
        d = _dist2(R[i], c)
        out[i] = d if first else min(float(d2[i]), d)
    return out


def chol_inverse(G, shift_rel=0.0):
    """-> (Rinv, pivots, diag): with A = (G + G^T) / 2 + shift_rel * mean(diag G) * I = L L^T, Rinv = (L^T)^-1 (upper triangular),
    pivots[i] = L[i, i]^2 and diag[i] = A[i, i].  Column-by-column Cholesky, then U X = I by back substitution with U = L^T."""
    G = np.asarray(G, dtype=np.float64)
    k = G.shape[0]
    s = 0.0
    for i in range(k):
        s += G[i, i]
    s *= shift_rel / k
    A = np.zeros((k, k))
    for i in range(k):
        for j in range(k):
            A[i, j] = 0.5 * (G[i, j] + G[j, i]) + (s if i == j else 0.0)
    L = np.zeros((k, k))
    piv = np.zeros(k)
    for j in range(k):
        p = A[j, j]
        for q in range(j):
            p -= L[j, q] * L[j, q]
        piv[j] = p
        if not p > 0.0:
            raise np.linalg.LinAlgError(f"chol_inverse: pivot {j} = {p} is not positive")
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, k):
            v = A[i, j]
            for q in range(j):
                v -= L[i, q] * L[j, q]
            L[i, j] = v / L[j, j]
    X = np.zeros((k, k))
    for col in range(k):                      # solve U x = e_col, U = L^T upper triangular: x[i] = 0 below the diagonal entry
        for i in range(col, -1, -1):
            v = 1.0 if i == col else 0.0
            for q in range(i + 1, col + 1):
                v -= L[q, i] * X[q, col]
            X[i, col] = v / L[i, i]
    return X, piv, np.diag(A).copy()


# ------------------------------------------------------------------ the one fp32 restatement
def block_sums_f32(R, labels, kc):
    """The per-block partial sums of kmeans_assign, exactly: for each block of 256 rows and each (cluster q, column c) ONE fp32 chain
    acc = acc + (label[r] == q ? R[r, c] : +0.0f) over the block's 256 row slots in ascending order, starting from +0.0f; slots past
    the last row hold label -1.  -> (part_sum fp32 [nb, kc, k], part_cnt int32 [nb, kc])."""
    R = np.asarray(R)
    assert R.dtype == np.float32
    labels = np.asarray(labels)
    n, k = R.shape
    nb = (n + BLOCK - 1) // BLOCK
    ps = np.zeros((nb, kc, k), dtype=np.float32)
    pc = np.zeros((nb, kc), dtype=np.int32)
    zero = np.zeros((kc, k), dtype=np.float32)
    q_of = np.arange(kc)
    for b in range(nb):
        acc = np.zeros((kc, k), dtype=np.float32)
        for slot in range(BLOCK):
            r = b * BLOCK + slot
            lab = int(labels[r]) if r < n else -1
            member = (q_of == lab)[:, None]
            row = R[r][None, :] if r < n else zero[:1]
            acc = (acc + np.where(member, row, zero)).astype(np.float32)      # fp32 + fp32 -> fp32, one rounding per step
            if 0 <= lab < kc:
                pc[b, lab] += 1
        ps[b] = acc
    return ps, pc


def bits(a):
    """The bit patterns of an fp32 array (so that -0.0 != +0.0 and NaN == NaN in a comparison)."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


# ------------------------------------------------------------------ bounds (derived; see tests/test_spectral_primitives_gpu.py)
def gram_bound(X, Y, G64):
    """A block is one fmaf chain of at most 256 terms (gamma_256 <= 256 u on sum |x||y|); blocks are summed in float64, rounded once."""
    return BLOCK * U24 * gram(np.abs(X), np.abs(Y)) + U24 * np.abs(G64)


def apply_bound(X, R, scale=None):
    """k fmaf steps and one multiplication by scale: (k + 1) u |scale_i| sum_a |x_ia||r_ac|."""
    k = np.asarray(X).shape[1]
    return (k + 1) * U24 * apply(np.abs(X), np.abs(R), None if scale is None else np.abs(scale))


def unit_bound(k):
    return (k + 4) * U24


def dist2_bound(k, d64):
    return (k + 3) * 2.0 ** -23 * np.asarray(d64, dtype=np.float64)


def decisive(k, d64, margin):
    """Rows whose float64 best-minus-second margin exceeds twice the dist2 bound: there the fp32 argmin cannot differ."""
    with np.errstate(invalid="ignore"):
        return margin > 2.0 * dist2_bound(k, d64)


# ------------------------------------------------------------------ shared cases and generators
N_SET = (1, 255, 256, 257, 513, 1000)
K_SET = (1, 2, 7, 16, 31, 32)
KC_SET = (1, 2, 31, 32)

# (n, k): rows_gram, rows_apply, rows_unit, kmeans_mindist
NK_CASES = [(1, 1), (1, 32), (255, 7), (255, 31), (256, 16), (256, 32), (257, 1), (257, 32), (513, 2), (513, 31), (1000, 16), (1000, 32)]
# (n, k, kc): kmeans_assign
NKC_CASES = [(1, 1, 1), (1, 32, 32), (255, 7, 2), (255, 31, 32), (256, 16, 31), (256, 32, 32), (257, 1, 2), (257, 32, 32), (257, 7, 1),
             (513, 2, 31), (513, 31, 2), (1000, 16, 32), (1000, 32, 31)]
INT_MAX = 7               # integer-exact inputs lie in [-7, 7]


def case_seed(*shape):
    """One seed per shape, the same in the CPU and the GPU file."""
    s = 20240
    for v in shape:
        s = s * 1009 + int(v)
    return s


def int_rows(n, k, seed, amax=INT_MAX):
    return np.random.default_rng(seed).integers(-amax, amax + 1, size=(n, k)).astype(np.float32)


def real_rows(n, k, seed):
    return np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)


def pow2_scale(n, seed):
    """Per-row scales 2^e, e in -3 .. 3, either sign: multiplying by one is exact."""
    rng = np.random.default_rng(seed)
    return (np.ldexp(1.0, rng.integers(-3, 4, size=n)) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


def label_case(n, k, kc):
    """The real-valued k-means case of a shape: rows and centres from one seeded gaussian."""
    seed = case_seed(n, k, kc)
    return real_rows(n, k, seed), real_rows(kc, k, seed + 1)


def int_label_case(n, k, kc):
    seed = case_seed(n, k, kc) + 7
    return int_rows(n, k, seed), int_rows(kc, k, seed + 1)
