"""Engine's clustering calls: the spectral pieces (the rectified-affinity mat-vec, the C spectral driver and the thin [n, k] helpers), both
centroid linkages, the device k-means, the PLDA transform with VBx and its centroids, and the streaming diarization's speaker tracking.

ClusterMixin is a mixin of ops.Engine: no state and no __init__ of its own.  It uses self.lib, self.ctx, self.device, self._workspace
only, and this module imports ops.py for nothing (ops.py imports it).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _args
from ._args import THIN_MAX
from ._lib import check
from .ops_util import _need, _ptr, _stream

STREAM_RING = 1024       # SDK_STREAM_RING: frames a stream's ring holds, and the most a step emits


class StreamState:
    """Engine.stream_state: the opaque device block of a bank of live streams (buf) and the rows its steps write."""

    def __init__(self, eng, R: int, capacity: int, d: int, nbytes: int):
        dev = eng.device
        self.R, self.capacity, self.d, self.nbytes = R, capacity, d, nbytes
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.labels = torch.full((R, 3), -1, dtype=torch.int32, device=dev)
        self.score = torch.zeros((R, 3), dtype=torch.float32, device=dev)
        self.K = torch.zeros((R,), dtype=torch.int32, device=dev)
        self.emit_lo = torch.zeros((R,), dtype=torch.int64, device=dev)
        self.emit_n = torch.zeros((R,), dtype=torch.int32, device=dev)
        self.count = torch.zeros((R, STREAM_RING), dtype=torch.uint8, device=dev)
        self.speakers = torch.full((R, STREAM_RING, 2), -1, dtype=torch.int32, device=dev)


def _picked_rows(who: str, E, rows, check_rows: bool) -> int:
    """E [R, d] fp32 rows and rows [n] int32, the rows of E a kernel reads (plda_transform, vbx_centroids, kmeans_rows) -> n.  The range
    check reads rows back, which waits for the device."""
    _args.rows(who, "E", E)
    n = int(_args.tensor(who, "rows", rows, "int32", (None,)).numel())
    if n < 1 or n > 65536:
        raise ValueError(f"{who}: n={n} rows (1 .. 65536)")
    if check_rows and not (0 <= int(rows.min()) and int(rows.max()) < E.shape[0]):      # the kernels read E at these rows
        raise ValueError(f"{who}: rows must lie in [0, {E.shape[0]}), got {int(rows.min())} .. {int(rows.max())}")
    return n


def _linkage_offsets(who: str, offsets, N: int):
    """The row bounds of a linkage's problems (None: one problem of all N rows) -> (off int64, off32, G, off32's pointer)."""
    off = np.asarray([0, N] if offsets is None else offsets, dtype=np.int64)
    if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != N:
        raise ValueError(f"{who}: offsets must run from 0 to N = {N}, got {off.tolist()[:8]}")
    off32 = np.ascontiguousarray(off.astype(np.int32))
    return off, off32, off32.size - 1, off32.ctypes.data_as(C.POINTER(C.c_int32))


def _linkage_status(who: str, off, status, Z, merges=None) -> None:
    """Read a linkage's status [G] back; a problem with a non-finite row raises ValueError naming the first one, with .linkage (the other
    problems' rows of Z are valid), .status and, for the linked linkage, .merges."""
    st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if bad.size:
        g = int(bad[0])
        err = ValueError(f"{who}: problem {g} (rows {int(off[g])} .. {int(off[g + 1])}) has a non-finite row or distance "
                         f"(status {int(st[g])}); problems with one: {bad.tolist()[:16]}")
        err.linkage, err.status = Z, st
        if merges is not None:
            err.merges = merges
        raise err


class ClusterMixin:
    # ------------------------------------------------------------------ k6 (spectral clustering pieces)
    def affinity_matvec(self, Eb, X, row0: int = 0, rows: Optional[int] = None, xscale=None, out=None):
        """Y[row0:row0+rows] = max(E E^T, 0)[row0:row0+rows, :] @ (xscale[:, None] * X);  X [N, kv] fp32."""
        _need(Eb, torch.bfloat16, "Eb"); _need(X, torch.float32, "X")
        N, d = Eb.shape
        kv = X.shape[1]
        rows = N - row0 if rows is None else rows
        Y = out if out is not None else torch.zeros((N, kv), dtype=torch.float32, device=self.device)
        ws = self._workspace("sdk_affinity_matvec_workspace_bytes", N, cache="matvec")
        check(self.lib.sdk_affinity_matvec(self.ctx, Eb.data_ptr(), N, d, row0, rows, X.contiguous().data_ptr(), _ptr(xscale), kv,
                                           Y.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdk_affinity_matvec")
        return Y

    def laplacian_topk(self, Eb_all, V0, n_iter: int, row0: int = 0, rows: Optional[int] = None, comm: Optional[int] = None, world: int = 1,
                       flag: Optional[torch.Tensor] = None):
        """The C-ABI spectral driver for non-Python hosts (sdk_laplacian_topk): top-k Ritz pairs of D^-1/2 A D^-1/2 by subspace iteration,
        never leaving the stream.  V0 [rows, k] fp32 start block (not modified) -> (U [rows, k], eigenvalues [k] device, descending).
        comm: an ncclComm_t as an integer (or None on one GPU)."""
        what = "laplacian_topk"
        # the C entry reads Eb_all as [N, 192] (the width the mat-vec kernel is built for) and V as [rows, k] through bare pointers:
        # everything it cannot see is refused here, before the scratch allocation and any launch
        N = int(_args.tensor(what, "Eb_all", Eb_all, "bfloat16", (None, 192)).shape[0])
        if N < 1:
            raise ValueError(f"{what}: Eb_all must be [N, 192] with N >= 1, got {list(Eb_all.shape)}")
        if not (isinstance(row0, (int, np.integer)) and row0 >= 0):
            raise ValueError(f"{what}: row0 = {row0!r} must be an integer >= 0")
        rows = N - row0 if rows is None else rows
        if not (isinstance(rows, (int, np.integer)) and rows >= 1):
            raise ValueError(f"{what}: rows = {rows!r} must be an integer >= 1 (row0 = {row0}, N = {N})")
        if row0 + rows > N:
            raise ValueError(f"{what}: row0 + rows = {row0 + rows} exceeds the N = {N} rows of Eb_all")
        k = int(_args.tensor(what, "V0", V0, "float32", (rows, None), contiguous=False).shape[1])      # one row per owned row of Eb_all
        if not 1 <= k <= THIN_MAX:
            raise ValueError(f"{what}: V0 must be [rows, k] with k in 1..{THIN_MAX}, got {list(V0.shape)}")
        if not (isinstance(n_iter, (int, np.integer)) and n_iter >= 0):
            raise ValueError(f"{what}: n_iter = {n_iter!r} must be an integer >= 0")
        if flag is not None and _args.tensor(what, "flag", flag, "int32").numel() != 1:
            raise ValueError(f"{what}: flag must hold one int32, got shape {list(flag.shape)}")
        V = V0.contiguous().clone()
        lam = torch.empty((k,), dtype=torch.float32, device=self.device)
        ws = self._workspace("sdk_laplacian_topk_workspace_bytes", N, k, cache="laplacian")
        check(self.lib.sdk_laplacian_topk(self.ctx, Eb_all.data_ptr(), N, row0, rows, k, n_iter, V.data_ptr(), lam.data_ptr(), _ptr(flag), ws.data_ptr(),
                                          ws.numel(), comm, world, _stream()), "sdk_laplacian_topk")
        return V, lam

    def rows_gram(self, X, Y):
        """G [k, k] = X^T Y over the n rows of two contiguous fp32 [n, k] blocks (k <= 32)."""
        n, k = _args.thin("rows_gram", "X", X)
        _args.tensor("rows_gram", "Y", Y, "float32", (n, k))
        G = torch.empty((k, k), dtype=torch.float32, device=self.device)
        ws = self._workspace("sdk_rows_gram_workspace_bytes", n, k, cache="gram")
        check(self.lib.sdk_rows_gram(self.ctx, X.data_ptr(), Y.data_ptr(), n, k, G.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdk_rows_gram")
        return G

    def rows_apply(self, X, R, scale=None):
        """Y[i, :] = scale[i] * (X[i, :] @ R): X contiguous fp32 [n, k], R fp32 [k, k], scale fp32 [n] or None."""
        n, k = _args.thin("rows_apply", "X", X)
        _args.tensor("rows_apply", "R", R, "float32", (k, k), contiguous=False)
        if scale is not None:
            _args.tensor("rows_apply", "scale", scale, "float32", (n,))
        Y = torch.empty_like(X)
        check(self.lib.sdk_rows_apply(self.ctx, X.data_ptr(), R.contiguous().data_ptr(), _ptr(scale), n, k, Y.data_ptr(), _stream()), "sdk_rows_apply")
        return Y

    def chol_inverse(self, G, flag: Optional[torch.Tensor] = None):
        """Rinv [k,k] with (G+G^T)/2 = L L^T, Rinv = (L^T)^-1 (float64 inside, stays on the stream).  `flag` (device int32 [1], zeroed
        by the caller) is set to 1 when G is not positive definite (rank-deficient or NaN input); it is sticky, so one flag can watch a
        whole iteration and be read at the caller's next host synchronisation."""
        k = G.shape[0]
        if flag is not None:
            _need(flag, torch.int32, "flag")
        Rinv = torch.empty((k, k), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_chol_inverse(self.ctx, G.contiguous().data_ptr(), k, Rinv.data_ptr(), _ptr(flag), _stream()), "sdk_chol_inverse")
        return Rinv

    def sym_eigh(self, G):
        """(Q [k, k], lam [k]) fp32 on the device: every eigenpair of (G + G^T) / 2 for a contiguous fp32 G [k, k], 1 <= k <= 32 - the Ritz
        step of laplacian_topk alone (sdk_sym_eigh: cyclic Jacobi in float64, stays on the stream).  lam descending, equal eigenvalues in
        ascending order of their diagonal position; column c of Q belongs to lam[c], with its largest-magnitude component positive."""
        k = int(_args.tensor("sym_eigh", "G", G, "float32", (None, None)).shape[0])
        if G.shape[1] != k:
            raise ValueError(f"sym_eigh: G must be square [k, k], got {list(G.shape)}")
        if not 1 <= k <= THIN_MAX:
            raise ValueError(f"sym_eigh: k = {k} (the order of G) must be in 1..{THIN_MAX}")
        Q = torch.empty((k, k), dtype=torch.float32, device=self.device)
        lam = torch.empty((k,), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_sym_eigh(self.ctx, G.data_ptr(), k, Q.data_ptr(), lam.data_ptr(), _stream()), "sdk_sym_eigh")
        return Q, lam

    def rows_unit(self, X):
        """The rows of a contiguous fp32 [n, k] block scaled to unit length (a row shorter than 1e-12 is divided by 1e-12: a zero row stays zero)."""
        n, k = _args.thin("rows_unit", "X", X)
        Y = torch.empty_like(X)
        check(self.lib.sdk_rows_unit(self.ctx, X.data_ptr(), n, k, Y.data_ptr(), _stream()), "sdk_rows_unit")
        return Y

    def kmeans_mindist(self, R, centre, d2, first: bool):
        """d2[i] = |R[i] - centre|^2 (first) or min(d2[i], that), in place: R contiguous fp32 [n, k], centre fp32 [k], d2 contiguous fp32 [n]."""
        n, k = _args.thin("kmeans_mindist", "R", R)
        _args.tensor("kmeans_mindist", "centre", centre, "float32", (k,), contiguous=False)
        _args.tensor("kmeans_mindist", "d2", d2, "float32", (n,))
        check(self.lib.sdk_kmeans_mindist(self.ctx, R.data_ptr(), n, k, centre.contiguous().data_ptr(), d2.data_ptr(), int(first), _stream()), "sdk_kmeans_mindist")
        return d2

    def kmeans_assign(self, R, centres, want_sums: bool = True):
        """One k-means step on the contiguous fp32 rows R [n, k] against centres fp32 [kc, k] (k, kc <= 32) ->
        (label int32 [n], dist2 fp32 [n], part_sum fp32 [ceil(n / 256), kc, k], part_cnt int32 [ceil(n / 256), kc]); the last two are None
        without want_sums.  label is the nearest centre, ties to the lowest index; part_sum / part_cnt are the sums and counts of each
        block of 256 rows per label, added in ascending row order (reproducible).
        A row that holds a NaN (or whose distance to every centre is NaN, as with NaN centres) compares below nothing: it gets label -1 and
        dist2 +inf and enters no sum and no count; the other rows of its block are not affected.  cluster.canonical_labels refuses a
        negative label."""
        n, k = _args.thin("kmeans_assign", "R", R)
        kc = int(_args.tensor("kmeans_assign", "centres", centres, "float32", (None, k), contiguous=False).shape[0])   # k: the width of R
        if not 1 <= kc <= THIN_MAX:
            raise ValueError(f"kmeans_assign: kc = {kc} (the rows of centres) must be in 1..{THIN_MAX}")
        lab = torch.empty((n,), dtype=torch.int32, device=self.device)
        d2 = torch.empty((n,), dtype=torch.float32, device=self.device)
        nb = (n + 255) // 256
        ps = torch.empty((nb, kc, k), dtype=torch.float32, device=self.device) if want_sums else None
        pc = torch.empty((nb, kc), dtype=torch.int32, device=self.device) if want_sums else None
        check(self.lib.sdk_kmeans_assign(self.ctx, R.data_ptr(), n, k, centres.contiguous().data_ptr(), kc, lab.data_ptr(), d2.data_ptr(),
                                         _ptr(ps), _ptr(pc), _stream()), "sdk_kmeans_assign")
        return lab, d2, ps, pc

    # ------------------------------------------------------------------ k6 (threshold path: centroid-linkage agglomerative clustering)
    def centroid_linkage(self, E: torch.Tensor, offsets=None) -> torch.Tensor:
        """E [N, d] fp32 unit rows (device) -> Z float64 [N - G, 4] (device): scipy's centroid linkage of every problem, in its layout and
        numbering.  offsets (host, G + 1 strictly increasing row bounds; None = one problem of all N rows): problem g's n_g - 1 rows start at
        row offsets[g] - g.  Raises ValueError naming the problem when one holds a non-finite row (its rows of Z are then not written; the
        exception carries .linkage, with the other problems' rows valid, and .status [G])."""
        _need(E, torch.float32, "E")
        if E.dim() != 2 or E.stride(1) != 1:
            E = E.contiguous()
        N, d = E.shape
        off, off32, G, op = _linkage_offsets("centroid_linkage", offsets, N)
        ws = self._workspace("sdk_centroid_linkage_workspace_bytes", op, G, d)
        Zbuf = torch.empty((max(N - G, 1), 4), dtype=torch.float64, device=self.device)   # never a null pointer (G single-row problems: no rows)
        status = torch.empty((G,), dtype=torch.int32, device=self.device)
        check(self.lib.sdk_centroid_linkage(self.ctx, E.data_ptr(), E.stride(0), d, op, G, Zbuf.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _stream()), "sdk_centroid_linkage")
        Z = Zbuf[:N - G]
        _linkage_status("centroid_linkage", off, status, Z)
        return Z

    def linked_linkage(self, E: torch.Tensor, group: torch.Tensor, offsets=None, stop=None):
        """E [N, d] fp32 unit rows, group [N] int32 (device) -> (Z float64 [N - G, 4], merges int32 [G]) on the device: the linked centroid
        linkage of every problem (sdk_linked_linkage; the rule heads csrc/ahc.hip).  Rows of one problem that share a group >= 0 never
        share a cluster (a negative group is a free row); each step merges the allowed pair of least centroid distance and the problem ends
        when none is left or that distance exceeds stop (None: +inf).  Problem g's rows of Z start at offsets[g] - g as in centroid_linkage;
        the rows from merges[g] on are zero.  Raises ValueError naming the problem when one holds a non-finite row, as centroid_linkage
        does (.linkage, .merges and .status on the exception)."""
        _need(E, torch.float32, "E")
        _need(group, torch.int32, "group")
        if E.dim() != 2 or E.stride(1) != 1:
            E = E.contiguous()
        N, d = E.shape
        if group.dim() != 1 or group.numel() != N:
            raise ValueError(f"linked_linkage: group must be [N] = [{N}], got {list(group.shape)}")
        group = group.contiguous()
        stop = float("inf") if stop is None else float(stop)
        if not stop >= 0.0:
            raise ValueError(f"linked_linkage: stop={stop} (a distance >= 0, or None / +inf for every allowed merge)")
        off, off32, G, op = _linkage_offsets("linked_linkage", offsets, N)
        ws = self._workspace("sdk_linked_linkage_workspace_bytes", op, G, d)
        Zbuf = torch.empty((max(N - G, 1), 4), dtype=torch.float64, device=self.device)   # never a null pointer
        merges = torch.empty((G,), dtype=torch.int32, device=self.device)
        status = torch.empty((G,), dtype=torch.int32, device=self.device)
        check(self.lib.sdk_linked_linkage(self.ctx, E.data_ptr(), E.stride(0), d, group.data_ptr(), op, G, stop, Zbuf.data_ptr(), merges.data_ptr(),
                                          status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdk_linked_linkage")
        Z = Zbuf[:N - G]
        _linkage_status("linked_linkage", off, status, Z, merges)
        return Z, merges

    # ---- spherical k-means on unit rows (cluster.kmeans_cluster; csrc/kmeans.hip): the whole loop in one enqueue, nothing read back here
    def kmeans_rows(self, E: torch.Tensor, rows: torch.Tensor, k: int, max_iters: int = 20, check_rows: bool = True):
        """E [R, d] fp32 unit rows, rows [n] int32 ascending (device), 1 <= k <= min(n, 64) -> (labels [n] int32 in [0, k), not canonical,
        n_iter [1] int32, status [1] int32), all on the device and not read back: sdk_kmeans_rows (the rule: cluster.kmeans_cluster).  The
        caller reads n_iter and status once.  check_rows=False: the caller has checked that rows lie in [0, R)."""
        n = _picked_rows("kmeans_rows", E, rows, check_rows)
        k, max_iters, d = int(k), int(max_iters), int(E.shape[1])
        if k < 1 or k > min(n, 64):
            raise ValueError(f"kmeans_rows: k={k} (1 .. min(n, 64), n={n})")
        if max_iters < 1 or max_iters > 1000:
            raise ValueError(f"kmeans_rows: max_iters={max_iters} (1 .. 1000)")
        ws = self._workspace("sdk_kmeans_rows_workspace_bytes", n, d, k)
        dev = E.device
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        n_iter = torch.empty((1,), dtype=torch.int32, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        check(self.lib.sdk_kmeans_rows(self.ctx, E.data_ptr(), rows.data_ptr(), n, d, k, max_iters, labels.data_ptr(), n_iter.data_ptr(),
                                       status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdk_kmeans_rows")
        return labels, n_iter, status

    # ---- VBx clustering (cluster.vbx_cluster, plda.py; csrc/vbx.hip): nothing here synchronises with the host except the range check of rows
    def plda_transform(self, E: torch.Tensor, rows: torch.Tensor, plda, check_rows: bool = True) -> torch.Tensor:
        """E [R, d_in] fp32 unit rows, rows [n] int32 (device), plda a plda.Plda -> X [n, D] float64 (device): sdk_plda_transform.
        check_rows=False: the caller has checked that rows lie in [0, R) (the check reads them back)."""
        n = _picked_rows("plda_transform", E, rows, check_rows)
        if int(E.shape[1]) != plda.d_in:
            raise ValueError(f"plda_transform: E has d={E.shape[1]}, the PLDA model takes d_in={plda.d_in}")
        D = int(plda.lda_dim)
        if D not in (64, 128) or D > plda.D0:
            raise ValueError(f"plda_transform: D={D} not supported (64 or 128, at most D0={plda.D0})")
        m = plda.device_arrays(E.device)
        X = torch.empty((n, D), dtype=torch.float64, device=E.device)
        check(self.lib.sdk_plda_transform(self.ctx, E.data_ptr(), plda.d_in, rows.data_ptr(), n, m["mean1"].data_ptr(), m["lda"].data_ptr(),
                                          m["mean2"].data_ptr(), m["mu"].data_ptr(), m["Tt"].data_ptr(), plda.D0, D, X.data_ptr(), _stream()),
              "sdk_plda_transform")
        return X

    def vbx(self, X: torch.Tensor, Phi: torch.Tensor, labels: torch.Tensor, S: int, Fa: float = 0.07, Fb: float = 0.8, max_iters: int = 20,
            epsilon: float = 1e-4, init_smoothing: float = 7.0):
        """X [n, D] float64, Phi [D] float64, labels [n] int32 in [0, S) (all on the device) -> (gamma [n, S], pi [S], elbo [max_iters],
        n_iter [1] int32, status [1] int32), all on the device and not read back: sdk_vbx.  The caller reads n_iter and status once."""
        return self._vbx("vbx", None, X, Phi, labels, S, Fa, Fb, max_iters, epsilon, init_smoothing)

    def vbx_hmm(self, X: torch.Tensor, Phi: torch.Tensor, labels: torch.Tensor, S: int, loop_prob: float, Fa: float = 0.07, Fb: float = 0.8,
                max_iters: int = 20, epsilon: float = 1e-4, init_smoothing: float = 7.0):
        """vbx with the HMM: the rows of X are a sequence in time order and loop_prob in [0, 1) is the probability that a row keeps the speaker
        of the row before it (sdk_vbx_hmm).  The same five device tensors."""
        loop_prob = float(loop_prob)
        if not 0.0 <= loop_prob < 1.0:                                    # a NaN fails both
            raise ValueError(f"vbx_hmm: loop_prob={loop_prob} (at least 0, below 1)")
        return self._vbx("vbx_hmm", loop_prob, X, Phi, labels, S, Fa, Fb, max_iters, epsilon, init_smoothing)

    def _vbx(self, who, loop_prob, X, Phi, labels, S, Fa, Fb, max_iters, epsilon, init_smoothing):
        n, D = (int(v) for v in _args.tensor(who, "X", X, "float64", (None, None)).shape)
        if D not in (64, 128):
            raise ValueError(f"{who}: D={D} not supported (64 or 128)")
        if n < 1 or n > 65536:
            raise ValueError(f"{who}: n={n} rows (1 .. 65536)")
        _args.tensor(who, "Phi", Phi, "float64", (D,))
        _args.tensor(who, "labels", labels, "int32", (n,))
        S, max_iters = int(S), int(max_iters)
        if S < 1 or S > 65536:
            raise ValueError(f"{who}: S={S} (1 .. 65536)")
        if max_iters < 1 or max_iters > 1000:
            raise ValueError(f"{who}: max_iters={max_iters} (1 .. 1000)")
        Fa, Fb, epsilon, init_smoothing = float(Fa), float(Fb), float(epsilon), float(init_smoothing)
        if not (0 < Fa < np.inf and 0 < Fb < np.inf) or epsilon != epsilon or not (0 <= init_smoothing < np.inf):
            raise ValueError(f"{who}: Fa={Fa} Fb={Fb} (positive, finite), epsilon={epsilon} (not NaN), init_smoothing={init_smoothing} (finite, >= 0)")
        ws = self._workspace("sdk_vbx_workspace_bytes" if loop_prob is None else "sdk_vbx_hmm_workspace_bytes", n, D, S)
        dev = X.device
        gamma = torch.empty((n, S), dtype=torch.float64, device=dev)
        pi = torch.empty((S,), dtype=torch.float64, device=dev)
        elbo = torch.empty((max_iters,), dtype=torch.float64, device=dev)
        n_iter = torch.empty((1,), dtype=torch.int32, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        head = (self.ctx, X.data_ptr(), Phi.data_ptr(), labels.data_ptr(), n, D, S, Fa, Fb, max_iters, epsilon, init_smoothing)
        tail = (gamma.data_ptr(), pi.data_ptr(), elbo.data_ptr(), n_iter.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        if loop_prob is None:
            check(self.lib.sdk_vbx(*head, *tail), "sdk_vbx")
        else:
            check(self.lib.sdk_vbx_hmm(*head, loop_prob, *tail), "sdk_vbx_hmm")
        return gamma, pi, elbo, n_iter, status

    def vbx_centroids(self, gamma: torch.Tensor, pi: torch.Tensor, E: torch.Tensor, rows: torch.Tensor, check_rows: bool = True):
        """gamma [n, S], pi [S] float64, E [R, d] fp32 unit rows, rows [n] int32 (all on the device) -> (K [1] int32, keep [S] int32,
        labels [n] int32, cent [S, d] fp32, cent64 [S, d] float64) on the device: sdk_vbx_centroids.  Rows K.. of the centroids are zeros."""
        n = _picked_rows("vbx_centroids", E, rows, check_rows)
        S, d = int(_args.tensor("vbx_centroids", "gamma", gamma, "float64", (n, None)).shape[1]), int(E.shape[1])
        if S < 1:
            raise ValueError(f"vbx_centroids: gamma must be [{n}, S] with S >= 1, got {list(gamma.shape)}")
        _args.tensor("vbx_centroids", "pi", pi, "float64", (S,))
        dev = E.device
        K = torch.empty((1,), dtype=torch.int32, device=dev)
        keep = torch.empty((S,), dtype=torch.int32, device=dev)
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        cent = torch.zeros((S, d), dtype=torch.float32, device=dev)
        cent64 = torch.zeros((S, d), dtype=torch.float64, device=dev)
        check(self.lib.sdk_vbx_centroids(self.ctx, gamma.data_ptr(), pi.data_ptr(), E.data_ptr(), rows.data_ptr(), n, S, d, K.data_ptr(), keep.data_ptr(),
                                         labels.data_ptr(), cent.data_ptr(), cent64.data_ptr(), _stream()), "sdk_vbx_centroids")
        return K, keep, labels, cent, cent64

    # ---- streaming diarization (stream.py; csrc/stream.hip): a bank's speaker tables and frame rings live in one device block
    def stream_state(self, n_streams: int, capacity: int, d: int) -> "StreamState":
        """The device state of a bank of n_streams live streams (capacity speakers each, embedding width d), reset, with the output rows
        that stream_step and stream_flush write."""
        nbytes = int(self.lib.sdk_stream_state_bytes(int(n_streams), int(capacity), int(d)))
        if nbytes == 0:
            raise ValueError(f"stream_state: n_streams={n_streams} (at least 1), capacity={capacity} (1 .. 64), d={d} (a multiple of 64, at most 512)")
        st = StreamState(self, int(n_streams), int(capacity), int(d), nbytes)
        self.stream_reset(st)
        return st

    def stream_reset(self, st: "StreamState", which: Optional[torch.Tensor] = None) -> None:
        """Empty the speaker table and the ring of the streams with which[r] != 0 (uint8 [R], device); None: of every stream."""
        if which is not None:
            _args.tensor("stream_reset", "which", which, "uint8", (st.R,))
        check(self.lib.sdk_stream_reset(self.ctx, st.buf.data_ptr(), st.nbytes, st.R, st.capacity, st.d, _ptr(which), _stream()), "sdk_stream_reset")

    def stream_step(self, st: "StreamState", E: torch.Tensor, info: torch.Tensor, cls: torch.Tensor, starts: torch.Tensor, active: torch.Tensor,
                    hop: int, latency: int, delta_new: float = 1.0, max_speakers: Optional[int] = None,
                    n_end: Optional[torch.Tensor] = None) -> "StreamState":
        """One bank step (sdk_stream_step): stream r's chunk is E [3 r .. 3 r + 2] (unit fp32 rows), info [r] (int32 [3, 4]), cls [r] (uint8 [F])
        and starts [r] (int64, samples); streams with active [r] == 0 (uint8) are left alone.  hop and latency in samples.  n_end (int64 [R], or None): n_end [r] > 0 says
        that the chunk is stream r's last and where the stream ends; no frame beyond that end is emitted.  The results stand
        in st.labels, st.score, st.K, st.emit_lo, st.emit_n, st.count and st.speakers (device), rows of inactive streams untouched."""
        R, d = st.R, st.d
        _args.tensor("stream_step", "E", E, "float32", (3 * R, d))
        _args.tensor("stream_step", "info", info, "int32", (R, 3, 4))
        _args.tensor("stream_step", "cls", cls, "uint8", (R, None))
        _args.tensor("stream_step", "starts", starts, "int64", (R,))
        _args.tensor("stream_step", "active", active, "uint8", (R,))
        if n_end is not None:
            _args.tensor("stream_step", "n_end", n_end, "int64", (R,))
        cap = 2 if max_speakers is None else int(max_speakers)
        check(self.lib.sdk_stream_step(self.ctx, E.data_ptr(), info.data_ptr(), cls.data_ptr(), starts.data_ptr(), active.data_ptr(), _ptr(n_end), R, int(cls.shape[1]),
                                       d, st.capacity, int(hop), int(latency), float(delta_new), cap, st.buf.data_ptr(), st.nbytes,
                                       st.labels.data_ptr(), st.score.data_ptr(), st.K.data_ptr(), st.emit_lo.data_ptr(), st.emit_n.data_ptr(),
                                       st.count.data_ptr(), st.speakers.data_ptr(), _stream()), "sdk_stream_step")
        return st

    def stream_flush(self, st: "StreamState", n_samples: torch.Tensor, active: torch.Tensor, max_speakers: Optional[int] = None) -> "StreamState":
        """The end of the streams with active [r] != 0 at n_samples [r] (int64, device): every frame not yet emitted stands in st.emit_lo,
        st.emit_n, st.count and st.speakers (sdk_stream_flush)."""
        _args.tensor("stream_flush", "n_samples", n_samples, "int64", (st.R,))
        _args.tensor("stream_flush", "active", active, "uint8", (st.R,))
        cap = 2 if max_speakers is None else int(max_speakers)
        check(self.lib.sdk_stream_flush(self.ctx, n_samples.data_ptr(), active.data_ptr(), st.R, st.capacity, st.d, cap, st.buf.data_ptr(), st.nbytes,
                                        st.emit_lo.data_ptr(), st.emit_n.data_ptr(), st.count.data_ptr(), st.speakers.data_ptr(), _stream()),
              "sdk_stream_flush")
        return st

    def stream_centroids(self, st: "StreamState", first: int = 0, count: Optional[int] = None, sums: bool = False):
        """Of the streams first .. first + count - 1 (count None: to the last) -> (cent [count, capacity, d] fp32 unit rows, zero from K [r]
        on; counts [count, capacity] int32; K [count] int32) on the device; sums=True: and the float64 sums [count, capacity, d]."""
        count = st.R - int(first) if count is None else int(count)
        if not (0 <= int(first) and 1 <= count <= st.R - int(first)):
            raise ValueError(f"stream_centroids: streams first={first}, count={count} of {st.R}")
        cent = torch.empty((count, st.capacity, st.d), dtype=torch.float32, device=self.device)
        counts = torch.empty((count, st.capacity), dtype=torch.int32, device=self.device)
        K = torch.empty((count,), dtype=torch.int32, device=self.device)
        S = torch.empty((count, st.capacity, st.d), dtype=torch.float64, device=self.device) if sums else None
        check(self.lib.sdk_stream_centroids(self.ctx, st.buf.data_ptr(), st.nbytes, st.R, st.capacity, st.d, int(first), count, cent.data_ptr(),
                                            counts.data_ptr(), K.data_ptr(), _ptr(S), _stream()), "sdk_stream_centroids")
        return (cent, counts, K, S) if sums else (cent, counts, K)


# ---- the nearest-neighbour graph of cluster.nmesc_cluster (csrc/nmesc.hip): functions of an engine, as diarize_ops.py's wrappers are, so that
# ops.Engine's public names stay the ones tests/test_ops_layout_cpu.py lists.  Only knn_rows, knn_rows_fused and knn_reverse read a status back.

def knn_rows(eng, E: torch.Tensor):
    """E [n, d] fp32 unit rows (device), 2 <= n <= 65536 -> (idx int32 [n, P], cos float64 [n, P]) on the device, P = min(KNN_P_MAX, n - 1):
    row i's P rows j != i of largest cosine, ties to the lower j, in that order (sdk_knn_rows; the cosine is the float64 sum of the exact
    products in column order).  One host read, the status: a row that holds a non-finite value raises ValueError naming the first one
    (.idx, .cos and .status on the exception; a NaN cosine ranks as -inf)."""
    n, d = _args.rows("knn_rows", "E", E)
    P = _args.knn_shape("knn_rows", n)
    idx = torch.empty((n, P), dtype=torch.int32, device=eng.device)
    cos = torch.empty((n, P), dtype=torch.float64, device=eng.device)
    status = torch.empty((2,), dtype=torch.int32, device=eng.device)
    check(eng.lib.sdk_knn_rows(eng.ctx, E.data_ptr(), n, d, P, idx.data_ptr(), cos.data_ptr(), status.data_ptr(), _stream()), "sdk_knn_rows")
    bad, first = (int(v) for v in status.cpu().numpy())
    if bad:
        err = ValueError(f"knn_rows: row {first} has a non-finite value ({bad} such rows in all)")
        err.idx, err.cos, err.status = idx, cos, (bad, first)
        raise err
    return idx, cos


def knn_rows_fused(eng, E_all: torch.Tensor, maps: torch.Tensor, weights):
    """The lists of a multi-scale affinity (cluster.nmesc_multiscale; sdk_knn_rows_fused): E_all [n_all, d] fp32 unit rows of every scale
    stacked (device), maps int32 [S, n] (device; base row i's row of E_all at scale s), weights S host numbers (finite, >= 0, not all
    zero; used as given) -> (idx int32 [n, P], cos float64 [n, P]) on the device: row i's P rows j != i of largest
    f(i, j) = sum over s in order of weights[s] * cosine(E_all[maps[s][i]], E_all[maps[s][j]]), ties to the lower j, and their f.  One host
    read, the status: a map entry outside [0, n_all) raises ValueError naming its base row (nothing is read through it; the lists are
    not to be trusted), and so does a row with a non-finite value that a map names (.idx, .cos and .status on the exception; a NaN f
    ranks as -inf).  A non-finite row no map names is not looked at."""
    n_all, d = _args.rows("knn_rows_fused", "E_all", E_all)
    S, n, P = _args.knn_maps("knn_rows_fused", maps)
    w = np.asarray(_args.knn_weights("knn_rows_fused", weights, S), dtype=np.float64)
    if n_all < 1 or n_all > _args.KNN_MAX_SCALES * 65536:
        raise ValueError(f"knn_rows_fused: E_all has {n_all} rows (1 .. {_args.KNN_MAX_SCALES * 65536})")
    idx = torch.empty((n, P), dtype=torch.int32, device=eng.device)
    cos = torch.empty((n, P), dtype=torch.float64, device=eng.device)
    status = torch.empty((4,), dtype=torch.int32, device=eng.device)
    check(eng.lib.sdk_knn_rows_fused(eng.ctx, E_all.data_ptr(), n_all, d, maps.data_ptr(), w.ctypes.data, S, n, P, idx.data_ptr(), cos.data_ptr(),
                                     status.data_ptr(), _stream()), "sdk_knn_rows_fused")
    bad, first, out, at = (int(v) for v in status.cpu().numpy())
    if out:
        raise ValueError(f"knn_rows_fused: base row {at} has a map entry outside [0, {n_all}) ({out} such entries in all)")
    if bad:
        err = ValueError(f"knn_rows_fused: row {first} of E_all, which a map names, has a non-finite value ({bad} such rows in all)")
        err.idx, err.cos, err.status = idx, cos, (bad, first)
        raise err
    return idx, cos


def knn_reverse(eng, idx: torch.Tensor, check_idx: bool = True):
    """idx int32 [n, P] (knn_rows') -> (rev_off int32 [n + 1], rev_src int32 [n P], rev_rank int32 [n P]) on the device: the incoming
    edges as CSR, row j's entries the rows that list j in ascending order with j's position in their lists (sdk_knn_reverse).  One host
    read, the status: an entry of idx outside [0, n) raises ValueError naming its row (the kernels skip such an entry).  check_idx=False:
    idx is knn_rows' own, nothing is read back."""
    n, P = _args.knn_lists("knn_reverse", idx)
    rev_off = torch.empty((n + 1,), dtype=torch.int32, device=eng.device)
    rev_src = torch.empty((n * P,), dtype=torch.int32, device=eng.device)
    rev_rank = torch.empty((n * P,), dtype=torch.int32, device=eng.device)
    status = torch.empty((2,), dtype=torch.int32, device=eng.device)
    ws = eng._workspace("sdk_knn_reverse_workspace_bytes", n, P)
    check(eng.lib.sdk_knn_reverse(eng.ctx, idx.data_ptr(), n, P, rev_off.data_ptr(), rev_src.data_ptr(), rev_rank.data_ptr(), status.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _stream()), "sdk_knn_reverse")
    bad, first = (int(v) for v in status.cpu().numpy()) if check_idx else (0, 0)
    if bad:
        raise ValueError(f"knn_reverse: row {first} of idx lists a row outside [0, {n}) ({bad} such entries in all)")
    return rev_off, rev_src, rev_rank


def knn_degree(eng, rev_off: torch.Tensor, rev_rank: torch.Tensor, P: int, p: int):
    """The graph pruned to the first p <= P neighbours -> (deg int32 [n], dinv float64 [n]) on the device: deg = p + the reverse entries
    of rank < p, dinv = 1 / sqrt(deg) (sdk_knn_degree).  Nothing is read back."""
    n = int(_args.tensor("knn_degree", "rev_off", rev_off, "int32", (None,)).numel()) - 1
    if _args.knn_shape("knn_degree", n) != int(P):
        raise ValueError(f"knn_degree: P={P} must be min({_args.KNN_P_MAX}, n - 1) = {_args.knn_shape('knn_degree', n)} (n={n})")
    _args.tensor("knn_degree", "rev_rank", rev_rank, "int32", (n * int(P),))
    _args.knn_p("knn_degree", p, P)
    deg = torch.empty((n,), dtype=torch.int32, device=eng.device)
    dinv = torch.empty((n,), dtype=torch.float64, device=eng.device)
    check(eng.lib.sdk_knn_degree(eng.ctx, rev_off.data_ptr(), rev_rank.data_ptr(), n, int(P), int(p), deg.data_ptr(), dinv.data_ptr(), _stream()),
          "sdk_knn_degree")
    return deg, dinv


def knn_matvec(eng, idx: torch.Tensor, rev, dinv: torch.Tensor, p: int, X: torch.Tensor):
    """Y = T_p X for X fp32 [n, kv], kv <= 32, T_p = (I + D^-1/2 A_p D^-1/2) / 2 over the lists idx, their reverse rev = (rev_off, rev_src,
    rev_rank) and dinv of knn_degree at the same p (sdk_knn_matvec; include/sdk_hip.h states the arithmetic operation by operation).
    Nothing is read back."""
    n, P = _args.knn_lists("knn_matvec", idx)
    rev_off, rev_src, rev_rank = rev
    _args.tensor("knn_matvec", "rev_off", rev_off, "int32", (n + 1,))
    _args.tensor("knn_matvec", "rev_src", rev_src, "int32", (n * P,))
    _args.tensor("knn_matvec", "rev_rank", rev_rank, "int32", (n * P,))
    _args.tensor("knn_matvec", "dinv", dinv, "float64", (n,))
    _args.knn_p("knn_matvec", p, P)
    _, kv = _args.thin("knn_matvec", "X", X)
    _args.tensor("knn_matvec", "X", X, "float32", (n, kv))
    Y = torch.empty_like(X)
    check(eng.lib.sdk_knn_matvec(eng.ctx, idx.data_ptr(), rev_off.data_ptr(), rev_src.data_ptr(), rev_rank.data_ptr(), dinv.data_ptr(), n, P,
                                  int(p), X.data_ptr(), kv, Y.data_ptr(), _stream()), "sdk_knn_matvec")
    return Y
