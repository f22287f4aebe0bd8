"""Symmetric adaptive score normalisation (AS-norm) of the identify / verify decision against a cohort of impostor embeddings.

The rule (this build's statement; parity with any outside toolkit is unpinned).  Inputs: unit fp32 rows E [N, d] (windows), P [Pn, d] (profiles),
Cn [M, d] (cohort) and an integer K, 1 <= K <= M.
  cohort statistics of a row x : of the M cosines <x, c_j> take the K largest (a multiset: equal scores need no tie rule); mean(x) is their
                                 mean, std(x) their population standard deviation (divide by K), floored at STD_FLOOR.
  normalised score             : z(n, p) = ((s - mean(e_n)) / std(e_n) + (s - mean(p)) / std(p)) / 2 with s = <e_n, p>.
  top-k over profiles          : the k <= 4 largest z per window, ties to the lowest profile index, each entry with its raw s beside its z.  A
                                 NaN z never wins; a window whose every z is NaN gets idx -1, score 0, raw 0.

On the device: ops.Engine.cohort_stats and ops.Engine.affinity_topk_snorm (csrc/snorm.hip: fp32 scores on the fp32-input MFMA, a radix select
per row, float64 statistics in a fixed order).  This module holds the cohort file (`Cohort`) and the rule's numpy float64 restatements
(`cohort_stats_host`, `snorm_topk_host`) for hosts that post-process stored embeddings; it imports neither torch nor the library.

The cohort file is a .npy [M, d] fp32 matrix, one embedding per impostor recording - `Backend.make_cohort` writes one: the unit mean embedding
`enroll_speaker` would store, per recording.  It is read through numpy's non-executing loader and its rows are normalised on the device.
"""
from __future__ import annotations

import hashlib
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

STD_FLOOR = 1e-6                  # floor of a row's cohort standard deviation (a cohort of equal scores must not divide by zero)
MAX_COHORT = 1 << 20              # cohort rows sdk_cohort_stats serves
MAX_TOPK = 4                      # k of the normalised top-k


class Cohort:
    """An impostor cohort: `matrix` [M, d] fp32 as stored, `digest` (content hash: names the statistics cached from it), `source` (its path).
    `device_rows(engine)` are its unit rows on the engine's device (Engine.l2norm, made once per engine)."""

    def __init__(self, matrix: np.ndarray, embedding_dim: Optional[int] = None, source: str = "<array>"):
        a = np.asarray(matrix)
        if a.ndim != 2:
            raise ValueError(f"cohort {source}: a [M, d] matrix expected, got an array of rank {a.ndim}, shape {tuple(a.shape)}")
        M, d = int(a.shape[0]), int(a.shape[1])
        if embedding_dim is not None and d != int(embedding_dim):
            raise ValueError(f"cohort {source}: rows of d={d}, the model's embedding_dim is {int(embedding_dim)}")
        if M < 1 or M > MAX_COHORT:
            raise ValueError(f"cohort {source}: M={M} rows (1 .. 2^20 = {MAX_COHORT})")
        if a.dtype.kind not in "fiu":
            raise ValueError(f"cohort {source}: a numeric matrix expected, got dtype {a.dtype}")
        a = np.ascontiguousarray(a, dtype=np.float32)
        if not np.isfinite(a).all():
            raise ValueError(f"cohort {source}: row {int(np.argwhere(~np.isfinite(a).all(axis=1))[0, 0])} holds a non-finite value")
        zero = ~a.any(axis=1)
        if zero.any():
            raise ValueError(f"cohort {source}: row {int(np.argwhere(zero)[0, 0])} is a zero row (it has no direction)")
        self.matrix = a
        self.source = str(source)
        h = hashlib.sha256(np.asarray(a.shape, dtype=np.int64).tobytes())
        h.update(a.tobytes())
        self.digest = h.hexdigest()[:16]
        self._dev = None

    @classmethod
    def load(cls, path, embedding_dim: Optional[int] = None) -> "Cohort":
        """The .npy at `path`; its shape is checked from the header before the data are read."""
        path = Path(path)
        try:
            a = np.load(path, mmap_mode="r", allow_pickle=False)        # numpy's non-executing loader
        except (OSError, ValueError) as e:
            raise ValueError(f"cohort {path}: not a readable .npy matrix ({e})") from e
        if not isinstance(a, np.ndarray):
            raise ValueError(f"cohort {path}: a .npy matrix expected (got an archive)")
        return cls(a, embedding_dim, source=str(path))

    def __len__(self) -> int:
        return int(self.matrix.shape[0])

    @property
    def dim(self) -> int:
        return int(self.matrix.shape[1])

    def device_rows(self, eng):
        if self._dev is None or self._dev[0] is not eng:
            import torch
            self._dev = (eng, eng.l2norm(torch.from_numpy(self.matrix).to(eng.device))[0])
        return self._dev[1]


def _rows64(x, name: str) -> np.ndarray:
    a = np.asarray(x, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"{name}: a [rows, d] matrix expected, got shape {tuple(a.shape)}")
    return a


def cohort_stats_host(E, cohort, K: int) -> Tuple[np.ndarray, np.ndarray]:
    """The cohort statistics of the rows of E in numpy float64: (mean [N], std [N])."""
    E, Cn = _rows64(E, "cohort_stats_host: E"), _rows64(cohort, "cohort_stats_host: cohort")
    M, K = int(Cn.shape[0]), int(K)
    if E.shape[1] != Cn.shape[1]:
        raise ValueError(f"cohort_stats_host: E has d={E.shape[1]}, the cohort d={Cn.shape[1]}")
    if K < 1 or K > M:
        raise ValueError(f"cohort_stats_host: K={K} (1 .. M={M})")
    S = E @ Cn.T
    top = np.partition(S, M - K, axis=1)[:, M - K:]                     # the K largest of every row, in any order
    return top.mean(axis=1), np.maximum(top.std(axis=1), STD_FLOOR)


def snorm_topk_host(E, mean_e, std_e, P, mean_p, std_p, k: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The normalised top-k in numpy float64: (idx [N, k] int32, z [N, k], raw [N, k]); k at most min(4, Pn)."""
    E, P = _rows64(E, "snorm_topk_host: E"), _rows64(P, "snorm_topk_host: P")
    me, se = np.asarray(mean_e, np.float64).reshape(-1, 1), np.asarray(std_e, np.float64).reshape(-1, 1)
    mp, sp = np.asarray(mean_p, np.float64).reshape(1, -1), np.asarray(std_p, np.float64).reshape(1, -1)
    k = int(k)
    if k < 1 or k > MAX_TOPK or k > P.shape[0]:
        raise ValueError(f"snorm_topk_host: k={k} (1 .. min({MAX_TOPK}, Pn={P.shape[0]}))")
    if me.shape[0] != E.shape[0] or se.shape[0] != E.shape[0] or mp.shape[1] != P.shape[0] or sp.shape[1] != P.shape[0] or E.shape[1] != P.shape[1]:
        raise ValueError("snorm_topk_host: one statistic per row of E and of P, and one width, expected")
    S = E @ P.T
    with np.errstate(invalid="ignore", divide="ignore"):
        Z = 0.5 * ((S - me) / se + (S - mp) / sp)
    bad = np.isnan(Z)
    order = np.argsort(np.where(bad, np.inf, -Z), axis=1, kind="stable")[:, :k]          # NaN last; ties to the lower profile
    z, raw, lost = np.take_along_axis(Z, order, 1), np.take_along_axis(S, order, 1), np.take_along_axis(bad, order, 1)
    return np.where(lost, -1, order).astype(np.int32), np.where(lost, 0.0, z), np.where(lost, 0.0, raw)
