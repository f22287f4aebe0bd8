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

No trained PLDA is on hand: synthetic_plda makes a seeded, well-conditioned one, and PARITY WITH PYANNOTE IS UNPINNED, as for every model here.
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
