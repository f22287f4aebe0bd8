"""The PLDA model of the VBx clustering (cluster.vbx_cluster): the six arrays of the two public .npz files of the VBx recipe (Landini et
al., BUT) that PyAnnote's speaker-diarization-community-1 pipeline ships -

    xvec_transform.npz   mean1 [d_in], mean2 [D0], lda [d_in, D0]
    plda.npz             mu [D0], tr [D0, D0], psi [D0]

- and their load-time preparation, on the host in float64, once:

    W = inv(tr^T tr)            the within-speaker covariance
    B = inv((tr^T / psi) tr)    the between-speaker covariance
    B v = lambda W v            the generalised symmetric eigenproblem, v^T W v = 1 (what scipy.linalg.eigh(B, W) solves)
    Phi = the eigenvalues in descending order; T = the eigenvectors, transposed, in the same order; the first D = lda_dim of both are kept
    (D is 64 or 128, D <= D0)

The eigenproblem is solved by the Cholesky reduction (W = L L^T, eigh(L^-1 B L^-T), v = L^-T y), numpy only; each eigenvector's sign is fixed
so that its component of largest magnitude is positive.  scipy's solver may return the opposite sign for some: the iteration does not see it
(dimension d enters through x_d^2 and rho_d alpha_d, and alpha is linear in x).

The transform of an fp32 unit row e (sdk_plda_transform; transform_host restates it), unit(v) = v / max(|v|, 1e-300):

    x1 = sqrt(d_in) unit(e - mean1);  x2 = sqrt(D0) unit(lda^T x1 - mean2);  x = ((x2 - mu) T^T)[:D]

synthetic_plda makes a seeded, well-conditioned stand-in, and PARITY WITH PYANNOTE IS UNPINNED, as for every model here.  A model that knows the
embedding space it is used in is made by fit (statistics on the device, csrc/plda_fit.hip), fit_host (statistics in numpy) or
Backend.train_plda (from recordings with reference annotations), and written by save_plda in the two files above.

The training rule (PARITY WITH KALDI / BUT IS UNPINNED; the tests pin this statement).  Input: E [N, d_in] fp32 unit rows, labels [N] int32, a
class (speaker) id in [0, K) per row, D0 (the LDA width), lda_dim (64 or 128, <= D0), n_iters.  Classes without a row are ignored; K' is the
number of the others.  ValueError, before any launch that depends on it: a label outside [0, K) (it is never used as an index on the device),
K' < D0 + 1, N - K' < d_in, d_in not a multiple of 64 in 64 .. 512, D0 not in lda_dim .. min(d_in, 512).

  Stage 1.  mean1 = the mean of E's rows; x1 = sqrt(d_in) unit(e - mean1).  With the class counts n_k, class means m_k and overall mean m of x1:
      Sw = (1/N)(sum x1 x1^T - sum_k n_k m_k m_k^T),  Sb = (1/N) sum_k n_k (m_k - m)(m_k - m)^T;
      Sb v = lambda Sw v, v^T Sw v = 1, by the Cholesky reduction and the sign rule of prepare, eigenvalues descending; lda = the first D0
      eigenvectors [d_in, D0] (a Cholesky that fails: ValueError naming the within-class scatter); mean2 = lda^T m.
  Stage 2, on x2 = sqrt(D0) unit(lda^T x1 - mean2) (the two-covariance model, Kaldi's estimator).  mu = the mean of the class means of x2, each
      class weighing 1; S_off = sum x2 x2^T - sum_k n_k m_k m_k^T; W = B = I; per iteration Ws = S_off, wc = N - K', Bs = 0, bc = 0 and for each
      class  V = (B^-1 + n_k W^-1)^-1,  w = V n_k W^-1 (m_k - mu),  r = (m_k - mu) - w,  Bs += V + w w^T, bc += 1,  Ws += n_k V + n_k r r^T,
      wc += 1;  then W = Ws / wc, B = Bs / bc (classes of equal n_k share V).  Before each update the objective is reported:
      objf = sum_k -1/2 [logdet(B + W/n_k) + (m_k - mu)^T (B + W/n_k)^-1 (m_k - mu)] - 1/2 [(N - K') logdet W + tr(W^-1 S_off)].
  Output.  W = C C^T (Cholesky), eigh(C^-1 B C^-T) = U diag(s) U^T with s descending, psi = max(s, 1e-12), tr = U^T C^-1: then
      W = inv(tr^T tr) and B = inv((tr^T / psi) tr), which is what prepare rebuilds.

The sums over the N rows (class counts, class sums, total, scatter, of x1 and of x2) are the statistics; everything after them is fit_from_stats,
d x d solves on the host in float64, shared by fit and fit_host.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

LDA_DIMS = (64, 128)
MAX_DIM = 512                    # d_in (a multiple of 64) and D0 served by sdk_plda_transform


def prepare(tr: np.ndarray, psi: np.ndarray, lda_dim: int):
    """(tr [D0, D0], psi [D0]) -> (Phi [D] descending, T [D, D0]) in float64: the module docstring's preparation."""
    tr = np.asarray(tr, dtype=np.float64)
    psi = np.asarray(psi, dtype=np.float64)
    W = np.linalg.inv(tr.T @ tr)
    B = np.linalg.inv((tr.T / psi) @ tr)
    W, B = 0.5 * (W + W.T), 0.5 * (B + B.T)
    L = np.linalg.cholesky(W)
    Li = np.linalg.inv(L)
    C = Li @ B @ Li.T
    lam, Y = np.linalg.eigh(0.5 * (C + C.T))
    order = np.argsort(-lam, kind="stable")
    V = (Li.T @ Y)[:, order]                                             # columns: v^T W v = 1
    big = np.argmax(np.abs(V), axis=0)
    V = V * np.where(V[big, np.arange(V.shape[1])] < 0, -1.0, 1.0)[None, :]
    D = int(lda_dim)
    return np.ascontiguousarray(lam[order][:D]), np.ascontiguousarray(V.T[:D])


@dataclass
class Plda:
    mean1: np.ndarray             # [d_in]
    lda: np.ndarray               # [d_in, D0]
    mean2: np.ndarray             # [D0]
    mu: np.ndarray                # [D0]
    tr: np.ndarray                # [D0, D0]
    psi: np.ndarray               # [D0]
    lda_dim: int = 128
    Phi: np.ndarray = field(default=None, repr=False)      # [D] descending (prepared)
    T: np.ndarray = field(default=None, repr=False)        # [D, D0] (prepared)

    def __post_init__(self):
        for k in ("mean1", "lda", "mean2", "mu", "tr", "psi"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.float64))
        d_in, D0 = self.lda.shape if self.lda.ndim == 2 else (-1, -1)
        shapes = dict(mean1=(d_in,), mean2=(D0,), mu=(D0,), tr=(D0, D0), psi=(D0,))
        for k, want in shapes.items():
            if getattr(self, k).shape != want:
                raise ValueError(f"Plda: {k} has shape {getattr(self, k).shape}, {want} expected for lda {self.lda.shape}")
        if d_in < 64 or d_in % 64 or d_in > MAX_DIM or D0 > MAX_DIM:
            raise ValueError(f"Plda: d_in={d_in} (a multiple of 64, at most {MAX_DIM}) and D0={D0} (at most {MAX_DIM}) not supported")
        self.lda_dim = int(self.lda_dim)
        if self.lda_dim not in LDA_DIMS or self.lda_dim > D0:
            raise ValueError(f"Plda: lda_dim={self.lda_dim} not supported (64 or 128, at most D0={D0})")
        if not (np.isfinite(self.psi).all() and (self.psi > 0).all()):
            raise ValueError("Plda: psi must be finite and positive")
        if self.Phi is None or self.T is None:
            self.Phi, self.T = prepare(self.tr, self.psi, self.lda_dim)
        self._dev = {}

    @property
    def d_in(self) -> int:
        return int(self.lda.shape[0])

    @property
    def D0(self) -> int:
        return int(self.lda.shape[1])

    def device_arrays(self, device):
        """The prepared model as float64 tensors on `device` (uploaded once): mean1, lda, mean2, mu, Tt [D0, D], Phi."""
        import torch
        key = str(device)
        if key not in self._dev:
            host = dict(mean1=self.mean1, lda=self.lda, mean2=self.mean2, mu=self.mu, Tt=np.ascontiguousarray(self.T.T), Phi=self.Phi)
            self._dev[key] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.items()}
        return self._dev[key]

    def transform_host(self, E: np.ndarray) -> np.ndarray:
        """The transform of the module docstring in numpy (float64): E [n, d_in] -> X [n, D]."""
        def unit(v):
            return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-300)
        x1 = np.sqrt(float(self.d_in)) * unit(np.asarray(E, dtype=np.float64) - self.mean1)
        x2 = np.sqrt(float(self.D0)) * unit(x1 @ self.lda - self.mean2)
        return (x2 - self.mu) @ self.T.T


def load_plda(transform_npz, plda_npz, lda_dim: int = 128) -> Plda:
    """xvec_transform.npz (mean1, mean2, lda) and plda.npz (mu, tr, psi), in the public key names -> Plda (numpy's non-executing loader)."""
    with np.load(transform_npz, allow_pickle=False) as z:
        missing = [k for k in ("mean1", "mean2", "lda") if k not in z.files]
        if missing:
            raise ValueError(f"load_plda: {transform_npz} lacks {missing} (keys: {z.files})")
        mean1, mean2, lda = z["mean1"], z["mean2"], z["lda"]
    with np.load(plda_npz, allow_pickle=False) as z:
        missing = [k for k in ("mu", "tr", "psi") if k not in z.files]
        if missing:
            raise ValueError(f"load_plda: {plda_npz} lacks {missing} (keys: {z.files})")
        mu, tr, psi = z["mu"], z["tr"], z["psi"]
    return Plda(mean1, lda, mean2, mu, tr, psi, lda_dim)


def synthetic_plda(d_in: int, D0: int = 128, seed: int = 0, lda_dim: Optional[int] = None) -> Plda:
    """A seeded stand-in: small means, lda with orthonormal columns, tr = an orthogonal matrix with rows scaled within [0.7, 1.4]
    (cond(tr) = 2), psi positive and descending from 16 to 0.05.  lda_dim defaults to min(128, D0) rounded down to 64 or 128."""
    rng = np.random.default_rng(seed)
    d_in, D0 = int(d_in), int(D0)
    if D0 > d_in:
        raise ValueError(f"synthetic_plda: D0={D0} exceeds d_in={d_in}")
    lda = np.linalg.qr(rng.standard_normal((d_in, D0)))[0]
    Q = np.linalg.qr(rng.standard_normal((D0, D0)))[0]
    tr = Q * np.geomspace(1.4, 0.7, D0)[:, None]
    psi = np.geomspace(16.0, 0.05, D0)
    if lda_dim is None:
        lda_dim = 128 if D0 >= 128 else 64
    return Plda(0.02 * rng.standard_normal(d_in), lda, 0.02 * rng.standard_normal(D0), 0.05 * rng.standard_normal(D0), tr, psi, lda_dim)


# ------------------------------------------------------------------------------------------------ training (the module docstring's rule)
@dataclass
class PldaFit:
    """What a fit reports beside the model."""
    n_rows: int
    counts: np.ndarray            # [K] int64, rows per class id (0 for an unused id)
    n_classes: int                # K', the classes with a row
    eigenvalues: np.ndarray       # [d_in] stage 1, descending
    objf: np.ndarray              # [n_iters], before each update
    W: np.ndarray                 # [D0, D0] within-speaker covariance of x2
    B: np.ndarray                 # [D0, D0] between-speaker covariance of x2
    stats1: dict = field(default=None, repr=False)         # counts, sums, total, scatter of x1 (float64, host)
    stats2: dict = field(default=None, repr=False)         # the same of x2


def save_plda(plda: Plda, transform_npz, plda_npz) -> None:
    """Writes the six arrays under the public key names (xvec_transform.npz: mean1, mean2, lda; plda.npz: mu, tr, psi), float64, to exactly
    these paths; load_plda of them returns the arrays bit for bit."""
    with open(transform_npz, "wb") as f:
        np.savez(f, mean1=plda.mean1, mean2=plda.mean2, lda=plda.lda)
    with open(plda_npz, "wb") as f:
        np.savez(f, mu=plda.mu, tr=plda.tr, psi=plda.psi)


def check_fit_arguments(N: int, d_in: int, labels: np.ndarray, K: Optional[int], D0: int, lda_dim: int, n_iters: int):
    """The refusals of the rule, on the host, before anything runs -> (K, counts [K] int64, K')."""
    N, d_in, D0, lda_dim, n_iters = int(N), int(d_in), int(D0), int(lda_dim), int(n_iters)
    labels = np.asarray(labels)
    if labels.shape != (N,) or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"plda fit: labels must be {N} integers, got {labels.shape} {labels.dtype}")
    if d_in < 64 or d_in % 64 or d_in > MAX_DIM:
        raise ValueError(f"plda fit: d_in={d_in} not supported (a multiple of 64 in 64 .. {MAX_DIM})")
    if lda_dim not in LDA_DIMS:
        raise ValueError(f"plda fit: lda_dim={lda_dim} not supported (64 or 128)")
    if not lda_dim <= D0 <= min(d_in, MAX_DIM):
        raise ValueError(f"plda fit: D0={D0} must lie in lda_dim={lda_dim} .. min(d_in, {MAX_DIM})={min(d_in, MAX_DIM)}")
    if n_iters < 1:
        raise ValueError(f"plda fit: n_iters={n_iters} (at least 1)")
    if N < 1 or N > 1 << 24:
        raise ValueError(f"plda fit: N={N} rows (1 .. 2^24)")
    lo, hi = int(labels.min()), int(labels.max())
    K = hi + 1 if K is None else int(K)
    if lo < 0 or hi >= K:
        raise ValueError(f"plda fit: labels must lie in [0, {K}), got {lo} .. {hi}")
    counts = np.bincount(labels, minlength=K).astype(np.int64)
    Kp = int((counts > 0).sum())
    if Kp < D0 + 1:
        raise ValueError(f"plda fit: {Kp} classes with a row, at least D0 + 1 = {D0 + 1} needed")
    if N - Kp < d_in:
        raise ValueError(f"plda fit: N - K' = {N - Kp} within-class degrees of freedom, at least d_in = {d_in} needed")
    return K, counts, Kp


def _sym(A):
    return 0.5 * (A + A.T)


def _generalised_eigh(A, W, what):
    """A v = lambda W v, v^T W v = 1: prepare's Cholesky reduction and sign rule -> (lambda descending, V columns)."""
    try:
        L = np.linalg.cholesky(_sym(W))
    except np.linalg.LinAlgError as e:
        raise ValueError(f"plda fit: {what} is not positive definite (its Cholesky factorisation failed)") from e
    Li = np.linalg.inv(L)
    lam, Y = np.linalg.eigh(_sym(Li @ A @ Li.T))
    order = np.argsort(-lam, kind="stable")
    V = (Li.T @ Y)[:, order]
    big = np.argmax(np.abs(V), axis=0)
    V = V * np.where(V[big, np.arange(V.shape[1])] < 0, -1.0, 1.0)[None, :]
    return lam[order], V


def _host_stats(s):
    out = {k: np.asarray(s[k], dtype=np.int64 if k == "counts" else np.float64) for k in ("counts", "sums", "total", "scatter")}
    d = out["total"].shape[0]
    if out["sums"].shape != (len(out["counts"]), d) or out["scatter"].shape != (d, d):
        raise ValueError(f"plda fit: statistics of shapes {[out[k].shape for k in out]} do not belong together")
    return out


def fit_from_stats(total0, stats1_fn, stats2_fn, N: int, D0: int = 128, lda_dim: int = 128, n_iters: int = 10):
    """The host half of the rule, numpy float64.  total0 [d_in]: the sum of E's rows; stats1_fn(mean1) -> the statistics of x1 and
    stats2_fn(mean1, lda, mean2) -> those of x2, each a dict(counts [K], sums [K, d], total [d], scatter [d, d]).  -> (Plda, PldaFit)."""
    N, D0, n_iters = int(N), int(D0), int(n_iters)
    mean1 = np.asarray(total0, dtype=np.float64) / N
    d_in = mean1.shape[0]
    # stage 1
    s1 = _host_stats(stats1_fn(mean1))
    nz = s1["counts"] > 0
    n = s1["counts"][nz].astype(np.float64)
    Kp = int(nz.sum())
    mk = s1["sums"][nz] / n[:, None]
    m = s1["total"] / N
    Mw = mk * np.sqrt(n)[:, None]
    Sw = _sym(s1["scatter"] - Mw.T @ Mw) / N
    Mb = (mk - m[None, :]) * np.sqrt(n)[:, None]
    Sb = (Mb.T @ Mb) / N
    lam, V = _generalised_eigh(Sb, Sw, "the within-class scatter")
    lda = np.ascontiguousarray(V[:, :D0])
    mean2 = lda.T @ m
    # stage 2
    s2 = _host_stats(stats2_fn(mean1, lda, mean2))
    if not np.array_equal(s2["counts"], s1["counts"]):
        raise ValueError("plda fit: the two stages' class counts differ")
    mk = s2["sums"][nz] / n[:, None]
    mu = mk.sum(0) / Kp
    Mw = mk * np.sqrt(n)[:, None]
    S_off = _sym(s2["scatter"] - Mw.T @ Mw)
    dm = mk - mu[None, :]
    sizes, inverse = np.unique(s1["counts"][nz], return_inverse=True)
    W, B = np.eye(D0), np.eye(D0)
    objf = np.zeros(n_iters)
    for it in range(n_iters):
        Wi, Bi = np.linalg.inv(W), np.linalg.inv(B)
        Ws, Bs = S_off.copy(), np.zeros((D0, D0))
        f = -0.5 * ((N - Kp) * np.linalg.slogdet(W)[1] + np.trace(Wi @ S_off))
        for u, nk in enumerate(sizes):
            x = dm[inverse == u]                                          # the classes of nk rows share V
            nk = float(nk)
            T = _sym(B + W / nk)
            f += -0.5 * (len(x) * np.linalg.slogdet(T)[1] + np.einsum("ij,ij->", x @ np.linalg.inv(T), x))
            Vn = _sym(np.linalg.inv(Bi + nk * Wi))
            w = x @ (Vn @ (nk * Wi)).T
            r = x - w
            Bs += len(x) * Vn + w.T @ w
            Ws += len(x) * nk * Vn + nk * (r.T @ r)
        objf[it] = f
        W, B = _sym(Ws) / (N - Kp + Kp), _sym(Bs) / Kp
    try:
        Cf = np.linalg.cholesky(W)
    except np.linalg.LinAlgError as e:
        raise ValueError("plda fit: the within-speaker covariance W is not positive definite (its Cholesky factorisation failed)") from e
    Ci = np.linalg.inv(Cf)
    s, U = np.linalg.eigh(_sym(Ci @ B @ Ci.T))
    order = np.argsort(-s, kind="stable")
    psi = np.maximum(s[order], 1e-12)
    tr = U[:, order].T @ Ci
    model = Plda(mean1, lda, mean2, mu, tr, psi, lda_dim)
    return model, PldaFit(N, s1["counts"], Kp, lam, objf, W, B, s1, s2)


def _unit_rows(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-300)


def numpy_stats(X, labels, K):
    """Class counts, class sums, total and scatter of the float64 rows X in numpy (fit_host's statistics)."""
    X = np.asarray(X, dtype=np.float64)
    sums = np.zeros((K, X.shape[1]))
    np.add.at(sums, labels, X)
    return dict(counts=np.bincount(labels, minlength=K).astype(np.int64), sums=sums, total=X.sum(0), scatter=X.T @ X)


def fit_host(E, labels, D0: int = 128, lda_dim: int = 128, n_iters: int = 10, K: Optional[int] = None):
    """The rule with the statistics in numpy: E [N, d_in] unit rows, labels [N] in [0, K) (K defaults to the largest label + 1)
    -> (Plda, PldaFit).  For machines without a device, and the library's own restatement of fit."""
    E = np.asarray(E)
    if E.ndim != 2:
        raise ValueError(f"fit_host: E must be [N, d_in], got {E.shape}")
    N, d_in = E.shape
    labels = np.asarray(labels)
    K, _, _ = check_fit_arguments(N, d_in, labels, K, D0, lda_dim, n_iters)
    E64 = E.astype(np.float32).astype(np.float64)

    def x1(mean1):
        return np.sqrt(float(d_in)) * _unit_rows(E64 - mean1)

    def stats1(mean1):
        return numpy_stats(x1(mean1), labels, K)

    def stats2(mean1, lda, mean2):
        return numpy_stats(np.sqrt(float(D0)) * _unit_rows(x1(mean1) @ lda - mean2), labels, K)

    return fit_from_stats(E64.sum(0), stats1, stats2, N, D0, lda_dim, n_iters)


def fit(provider, E, labels, D0: int = 128, lda_dim: int = 128, n_iters: int = 10, K: Optional[int] = None):
    """The rule with the statistics on the device: provider an ops.Engine, E [N, d_in] fp32 unit rows and labels [N] int32 device tensors
    (K defaults to the largest label + 1) -> (Plda, PldaFit).  Four passes over the rows (the mean, the statistics of x1, the projection,
    the statistics of x2: sdk_plda_fit_stats, sdk_plda_project); the labels are read back once and checked before the first launch."""
    import torch
    if E.dim() != 2 or E.dtype != torch.float32 or not E.is_cuda:
        raise ValueError(f"fit: E must be an fp32 [N, d_in] device tensor, got {tuple(E.shape)} {E.dtype}")
    if labels.dtype != torch.int32 or not labels.is_cuda:
        raise ValueError(f"fit: labels must be an int32 device tensor, got {labels.dtype}")
    N, d_in = int(E.shape[0]), int(E.shape[1])
    K, _, _ = check_fit_arguments(N, d_in, labels.cpu().numpy(), K, D0, lda_dim, n_iters)
    E, labels = E.contiguous(), labels.contiguous()
    dev = E.device

    def host(s):
        if int(s["status"].item()):
            raise ValueError("fit: a label outside [0, K) reached the device")
        return {k: s[k].cpu().numpy() for k in ("counts", "sums", "total", "scatter")}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def stats1(mean1):
        return host(provider.plda_fit_stats(E, labels, K, mean1=up(mean1), check_labels=False))

    def stats2(mean1, lda, mean2):
        X2 = provider.plda_project(E, up(mean1), up(lda), up(mean2))
        return host(provider.plda_fit_stats(X2, labels, K, check_labels=False))

    total0 = provider.plda_fit_stats(E, scatter=False)["total"].cpu().numpy()
    return fit_from_stats(total0, stats1, stats2, N, D0, lda_dim, n_iters)


def plda_classes(recording, speaker, names, uris, speaker_key):
    """The class of every labelled row of Diarizer.plda_rows: (uri, reference name), numbered by first appearance, unless
    speaker_key(uri, name) maps several to one key; uri is the recording's entry of `uris`, else its index -> (labels int32, keys)."""
    keys: dict = {}
    labels = np.zeros(len(speaker), np.int32)
    for j, (r, s) in enumerate(zip(recording, speaker)):
        uri = uris[int(r)] if uris is not None else int(r)
        name = names[int(r)][int(s)]
        key = speaker_key(uri, name) if speaker_key is not None else (uri, name)
        labels[j] = keys.setdefault(key, len(keys))
    return labels, list(keys)
