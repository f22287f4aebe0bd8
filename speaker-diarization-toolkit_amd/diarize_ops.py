"""The device layer of the diarization: thin wrappers over sdk_powerset_decode and the sdk_diarize_* entry points of libsdk_hip.so
(csrc/diarize.hip), their argument checks, and GroupTables, the prefix-sum tables the grouped kernels search.  diarize.py states the rule and
diarize_host.py restates every kernel in numpy.  A leaf: it imports diarize_host.py, and _lib.py and ops.py at the first call; diarize.py,
cluster.py, score.py and stream.py import it, never the other way.  diarize.py re-exports every name."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _args
from .diarize_host import MAX_ASSIGN_DIM, N_LOCAL, _speaker_cap, global_frames

VBX_HOST_READS = 7              # cluster.vbx_cluster waits for the device 7 times: the linkage's status and Z, the one read (n_iter, status, K), labels, pi, elbo, keep
LINKAGE_HOST_READS = 1           # Engine.centroid_linkage reads its status back before it returns Z


def _native():
    """(torch, _lib.check, ops._stream), imported at the first call and not with this module: score.py's host path imports it and needs neither."""
    import torch
    from ._lib import check
    from .ops import _stream
    return torch, check, _stream


def _check_dim(name: str, d: int):
    _args.row_width(name, d, MAX_ASSIGN_DIM)


def _check_rows(name: str, E, rows: Optional[int] = None):
    """E: contiguous fp32 [rows, d] on the device (rows None: any count), d a width the assignment kernels serve -> (rows, d)."""
    return _args.rows(name, "E", E, n=rows, limit=MAX_ASSIGN_DIM)


def _check_tensor(name: str, what: str, t, dtype: str, shape: tuple, min_rows: int = 0, contiguous: bool = True):
    """The wrappers' check of cls (uint8 [C, F]), labels (int32 [C, 3]), info (int32 [C, 3, 4]), the centroids (float64 [K, d]) and the like:
    on the device, contiguous (contiguous=False: the wrapper passes t.contiguous() on), torch's dtype `dtype`, of `shape` (None: any size),
    at least min_rows rows."""
    if _args.tensor(name, what, t, dtype, shape, contiguous=contiguous).shape[0] < min_rows:
        raise ValueError(f"{name}: {what} must hold {min_rows} rows or more, got {list(t.shape)}")


def powerset_decode(eng, logp):
    """logp [C, F, 7] fp32 (device) -> cls [C, F] uint8 (device): sdk_powerset_decode."""
    torch, check, _stream = _native()
    _check_tensor("powerset_decode", "logp", logp, "float32", (None, None, 7), contiguous=False)
    logp = logp.contiguous()
    cls = torch.empty(logp.shape[:2], dtype=torch.uint8, device=logp.device)
    check(eng.lib.sdk_powerset_decode(eng.ctx, logp.data_ptr(), logp.shape[0], logp.shape[1], cls.data_ptr(), _stream()), "sdk_powerset_decode")
    return cls


def diarize_masks(eng, cls, T4: int):
    """cls [B, F] uint8 (device) -> (w [B, 3, T4] fp32, info [B, 3, 4] int32) on the device: sdk_diarize_masks."""
    torch, check, _stream = _native()
    _check_tensor("diarize_masks", "cls", cls, "uint8", (None, None))
    B, F = cls.shape
    w = torch.empty((B, N_LOCAL, T4), dtype=torch.float32, device=cls.device)
    info = torch.empty((B, N_LOCAL, 4), dtype=torch.int32, device=cls.device)
    check(eng.lib.sdk_diarize_masks(eng.ctx, cls.data_ptr(), B, F, int(T4), w.data_ptr(), info.data_ptr(), _stream()), "sdk_diarize_masks")
    return w, info


def diarize_reconstruct(eng, cls, starts, labels, K: int, n_samples: int, max_speakers: Optional[int] = None, want_act: bool = False):
    """cls [C, F] uint8, starts [C] int32 ascending, labels [C, 3] int32 (all on the device) -> (count [G] uint8, speakers [G, 2] int32,
    act [G, K] int32 or None) on the device: sdk_diarize_reconstruct."""
    torch, check, _stream = _native()
    _check_tensor("diarize_reconstruct", "cls", cls, "uint8", (None, None))
    Cn, F = cls.shape
    _check_tensor("diarize_reconstruct", "starts", starts, "int32", (Cn,), contiguous=False)
    _check_tensor("diarize_reconstruct", "labels", labels, "int32", (Cn, N_LOCAL), contiguous=False)
    starts, labels = starts.contiguous(), labels.contiguous()
    G = int(eng.lib.sdk_diarize_frames(int(n_samples)))
    count = torch.zeros((G,), dtype=torch.uint8, device=cls.device)
    speakers = torch.full((G, 2), -1, dtype=torch.int32, device=cls.device)
    act = torch.zeros((G, int(K)), dtype=torch.int32, device=cls.device) if want_act else None
    check(eng.lib.sdk_diarize_reconstruct(eng.ctx, cls.data_ptr(), starts.data_ptr(), labels.data_ptr(), Cn, F, int(K), int(n_samples),
                                          _speaker_cap(max_speakers), count.data_ptr(), speakers.data_ptr(), act.data_ptr() if want_act else None,
                                          _stream()), "sdk_diarize_reconstruct")
    return count, speakers, act


def diarize_centroids(eng, E, rows, labels, K: int, check_rows: bool = True):
    """E [R, d] fp32 unit rows, rows [n] int32 ascending, labels [n] int32 in [0, K) (all on the device) -> (cent [K, d] fp32 unit,
    cent64 [K, d] float64) on the device: sdk_diarize_centroids.  A cluster without rows gives a zero row.  check_rows=False: the caller
    has checked that rows lie in [0, R) (the check reads them back, which waits for the device)."""
    torch, check, _stream = _native()
    _check_rows("diarize_centroids", E)
    if int(K) < 1:
        raise ValueError(f"diarize_centroids: K={K} (at least 1)")
    _check_tensor("diarize_centroids", "rows", rows, "int32", (None,), contiguous=False)
    _check_tensor("diarize_centroids", "labels", labels, "int32", tuple(rows.shape), contiguous=False)
    rows, labels = rows.contiguous(), labels.contiguous()
    n, d = int(rows.numel()), int(E.shape[1])
    if check_rows and n and not (0 <= int(rows.min()) and int(rows.max()) < E.shape[0]):   # the kernel reads E at these rows
        raise ValueError(f"diarize_centroids: rows must lie in [0, {E.shape[0]}), got {int(rows.min())} .. {int(rows.max())}")
    cent = torch.empty((int(K), d), dtype=torch.float32, device=E.device)
    cent64 = torch.empty((int(K), d), dtype=torch.float64, device=E.device)
    check(eng.lib.sdk_diarize_centroids(eng.ctx, E.data_ptr(), rows.data_ptr(), labels.data_ptr(), n, int(K), d, cent.data_ptr(), cent64.data_ptr(),
                                        _stream()), "sdk_diarize_centroids")
    return cent, cent64


def diarize_assign(eng, E, info, cent, constrained: bool = False):
    """E [3 C, d] fp32 unit rows, info [C, 3, 4] int32, cent [K, d] float64 (diarize_centroids' second result), all on the device ->
    (labels [C, 3] int32, score [C, 3] fp32) on the device: sdk_diarize_assign."""
    torch, check, _stream = _native()
    n, d = _check_rows("diarize_assign", E)
    Cn = n // N_LOCAL
    if n != N_LOCAL * Cn:
        raise ValueError(f"diarize_assign: E must hold {N_LOCAL} rows per chunk, got {n} rows")
    _check_tensor("diarize_assign", "info", info, "int32", (Cn, N_LOCAL, 4))
    _check_tensor("diarize_assign", "the centroids", cent, "float64", (None, d))
    if cent.shape[0] < 1:
        raise ValueError("diarize_assign: K=0 (at least one centroid)")
    labels = torch.empty((Cn, N_LOCAL), dtype=torch.int32, device=E.device)
    score = torch.empty((Cn, N_LOCAL), dtype=torch.float32, device=E.device)
    check(eng.lib.sdk_diarize_assign(eng.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), Cn, int(cent.shape[0]), d, int(bool(constrained)),
                                     labels.data_ptr(), score.data_ptr(), _stream()), "sdk_diarize_assign")
    return labels, score


class GroupTables:
    """The prefix-sum tables of a pack on the host (checked here, once) and on the device (what the grouped kernels search).  uploads counts
    the host-to-device copies made so far."""

    def __init__(self, eng, chunk_off, frame_off, n_samples, starts_local=None):
        self.eng, self.uploads = eng, 0
        self.chunk_off, self.frame_off = np.asarray(chunk_off, dtype=np.int64), np.asarray(frame_off, dtype=np.int64)
        self.n_samples = np.asarray(n_samples, dtype=np.int64)
        self.R = R = int(self.n_samples.size)
        for name, off in (("chunk_off", self.chunk_off), ("frame_off", self.frame_off)):
            if R < 1 or off.shape != (R + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] >= (1 << 30):
                raise ValueError(f"GroupTables: {name} must hold R + 1 = {R + 1} prefix sums from 0 (below 2^30), got {off.tolist()[:8]}")
        if not np.array_equal(np.diff(self.frame_off), [global_frames(int(n)) for n in self.n_samples]):
            raise ValueError("GroupTables: frame_off must be the prefix sums of global_frames(n_samples)")
        self.C, self.G = int(self.chunk_off[-1]), int(self.frame_off[-1])
        parts = [self.chunk_off, self.frame_off] + ([np.asarray(starts_local, dtype=np.int64)] if starts_local is not None else [])
        if starts_local is not None and parts[2].shape != (self.C,):
            raise ValueError(f"GroupTables: starts_local must hold {self.C} chunk starts, got {parts[2].shape}")
        up = self._up(np.concatenate(parts).astype(np.int32))                                        # one upload
        self.chunk_off_d, self.frame_off_d = up[:R + 1], up[R + 1:2 * R + 2]
        self.starts_local_d = up[2 * R + 2:] if starts_local is not None else None
        self.n_samples_d = self._up(self.n_samples)
        self.cent_off = self.cent_off_d = self.act_off = self.act_off_d = None
        self.K = 0

    def _up(self, a: np.ndarray):
        self.uploads += 1
        return _native()[0].from_numpy(a).to(self.eng.device)

    def set_clusters(self, cent_off, want_act: bool = False):
        """cent_off [R + 1]: prefix sums of the recordings' cluster counts."""
        off = np.asarray(cent_off, dtype=np.int64)
        if off.shape != (self.R + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] >= (1 << 30):
            raise ValueError(f"GroupTables: cent_off must hold R + 1 = {self.R + 1} prefix sums from 0, got {off.tolist()[:8]}")
        self.cent_off, self.K = off, int(off[-1])
        self.cent_off_d = self._up(off.astype(np.int32))
        self.act_off = np.concatenate([[0], np.cumsum(np.diff(self.frame_off) * np.maximum(np.diff(off), 1))]).astype(np.int64)
        self.act_off_d = self._up(self.act_off) if want_act else None
        return self


def diarize_assign_grouped(eng, E, info, cent, tab: GroupTables, constrained: bool = False):
    """diarize_assign over a pack: cent [K, d] float64 holds recording r's centroids at tab.cent_off[r] .. tab.cent_off[r + 1] ->
    (labels [C, 3] int32 local to the recording, score [C, 3] fp32) on the device: sdk_diarize_assign_grouped."""
    torch, check, _stream = _native()
    _check_rows("diarize_assign_grouped", E, N_LOCAL * tab.C)
    Cn, d = tab.C, int(E.shape[1])
    _check_tensor("diarize_assign_grouped", "info", info, "int32", (Cn, N_LOCAL, 4))
    if tab.cent_off is None:
        raise ValueError("diarize_assign_grouped: the tables hold no clusters (set_clusters)")
    _check_tensor("diarize_assign_grouped", "the centroids", cent, "float64", (None, d), max(tab.K, 1))
    labels = torch.empty((Cn, N_LOCAL), dtype=torch.int32, device=E.device)
    score = torch.empty((Cn, N_LOCAL), dtype=torch.float32, device=E.device)
    check(eng.lib.sdk_diarize_assign_grouped(eng.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), tab.chunk_off_d.data_ptr(), tab.cent_off_d.data_ptr(),
                                             tab.R, Cn, d, int(bool(constrained)), labels.data_ptr(), score.data_ptr(), _stream()), "sdk_diarize_assign_grouped")
    return labels, score


def diarize_fold_grouped(eng, cent, sizes, cl_off, eff, cent_off, cut=None, upload=None):
    """The fold of cluster.fold_small_clusters over a pack, on the device: cent [Kc, d] float64 unit centroids of the cut (device), sizes
    [Kc], cl_off [R + 1], eff [R], cent_off [R + 1] (host integers; cent_off must count the large clusters of every recording, 1 when it has
    clusters and none is large), cut [n] int32 (device, or None): the cut's global cluster of every training row ->
    (remap [Kc] int32, out [n] int32 = remap[cut], or None) on the device: sdk_diarize_fold_grouped.  upload: what carries the one table of
    host integers to cent's device (a caller that counts its transfers passes its own)."""
    torch, check, _stream = _native()
    sizes, cl_off, eff, cent_off = (np.asarray(v, dtype=np.int64) for v in (sizes, cl_off, eff, cent_off))
    R, Kc = int(eff.size), int(sizes.size)
    large = None
    if R >= 1 and cl_off.shape == (R + 1,) and cl_off[0] == 0 and cl_off[-1] == Kc and (np.diff(cl_off) >= 0).all():
        rec = np.repeat(np.arange(R), np.diff(cl_off))                    # the recording of every cluster of the cut
        large = np.bincount(rec[sizes >= eff[rec]], minlength=R)
    if large is None or cent_off.shape != (R + 1,) or cent_off[0] != 0 or not np.array_equal(np.diff(cent_off), np.where(np.diff(cl_off) > 0, np.maximum(large, 1), 0)):
        raise ValueError("diarize_fold_grouped: cl_off must be the R + 1 prefix sums of the cut's cluster counts and cent_off those of the large clusters (1 when none)")
    _check_tensor("diarize_fold_grouped", "the centroids", cent, "float64", (None, None), Kc)
    d = int(cent.shape[1])
    _check_dim("diarize_fold_grouped", d)
    if cut is not None:
        _check_tensor("diarize_fold_grouped", "cut", cut, "int32", (None,))
    n = 0 if cut is None else int(cut.numel())
    up = (upload or (lambda a: torch.from_numpy(a).to(cent.device)))(np.concatenate([sizes, cl_off, eff, cent_off]).astype(np.int32))
    sizes_d, cl_d, eff_d, co_d = up[:Kc], up[Kc:Kc + R + 1], up[Kc + R + 1:Kc + 2 * R + 1], up[Kc + 2 * R + 1:]
    target = torch.empty((max(Kc, 1),), dtype=torch.int32, device=cent.device)
    remap = torch.empty((max(Kc, 1),), dtype=torch.int32, device=cent.device)
    out = torch.empty((max(n, 1),), dtype=torch.int32, device=cent.device)
    check(eng.lib.sdk_diarize_fold_grouped(eng.ctx, cent.data_ptr(), sizes_d.data_ptr(), cl_d.data_ptr(), eff_d.data_ptr(), co_d.data_ptr(), R, Kc, d,
                                           target.data_ptr(), remap.data_ptr(), cut.data_ptr() if n else None, n, out.data_ptr(), _stream()),
          "sdk_diarize_fold_grouped")
    return remap[:Kc], (out[:n] if cut is not None else None)


def diarize_reconstruct_grouped(eng, cls, labels, tab: GroupTables, max_speakers: Optional[int] = None, want_act: bool = False):
    """diarize_reconstruct over a pack: cls [C, F] uint8, labels [C, 3] int32 local to the recording (device), tab with starts_local and
    clusters set -> (count [G] uint8, speakers [G, 2] int32, act int32 [tab.act_off[-1]] or None) on the packed frame grid:
    sdk_diarize_reconstruct_grouped."""
    torch, check, _stream = _native()
    _check_tensor("diarize_reconstruct_grouped", "cls", cls, "uint8", (tab.C, None))
    _check_tensor("diarize_reconstruct_grouped", "labels", labels, "int32", (tab.C, N_LOCAL))
    if tab.starts_local_d is None or tab.cent_off is None or (want_act and tab.act_off_d is None):
        raise ValueError("diarize_reconstruct_grouped: the tables need starts_local and set_clusters (want_act=True for act)")
    count = torch.zeros((tab.G,), dtype=torch.uint8, device=cls.device)
    speakers = torch.full((tab.G, 2), -1, dtype=torch.int32, device=cls.device)
    act = torch.zeros((max(int(tab.act_off[-1]), 1),), dtype=torch.int32, device=cls.device) if want_act else None
    if tab.C and tab.G:
        check(eng.lib.sdk_diarize_reconstruct_grouped(eng.ctx, cls.data_ptr(), tab.starts_local_d.data_ptr(), labels.data_ptr(), tab.chunk_off_d.data_ptr(),
                                                      tab.frame_off_d.data_ptr(), tab.n_samples_d.data_ptr(), tab.cent_off_d.data_ptr(), tab.R, tab.C,
                                                      int(cls.shape[1]), tab.G, _speaker_cap(max_speakers), count.data_ptr(), speakers.data_ptr(),
                                                      act.data_ptr() if want_act else None, tab.act_off_d.data_ptr() if want_act else None, _stream()),
              "sdk_diarize_reconstruct_grouped")
    return count, speakers, act


def diarize_first_seen(eng, speakers, tab: GroupTables):
    """speakers [G, 2] int32 (device) -> first [K] int32 (device): sdk_diarize_first_seen (integer atomicMin)."""
    torch, check, _stream = _native()
    if tab.cent_off is None:
        raise ValueError("diarize_first_seen: the tables hold no clusters (set_clusters)")
    _check_tensor("diarize_first_seen", "speakers", speakers, "int32", (tab.G, 2))
    first = torch.empty((max(tab.K, 1),), dtype=torch.int32, device=speakers.device)
    check(eng.lib.sdk_diarize_first_seen(eng.ctx, speakers.data_ptr(), tab.frame_off_d.data_ptr(), tab.cent_off_d.data_ptr(), tab.R, tab.G, tab.K,
                                         first.data_ptr(), _stream()), "sdk_diarize_first_seen")
    return first[:tab.K]


def diarize_renumber(eng, first, labels, cent, cent64, tab: GroupTables):
    """first [K] (diarize_first_seen), labels [C, 3] int32 local (REWRITTEN in place), cent [K, d] fp32 and cent64 [K, d] float64 ->
    (renum [K] int32, cent and cent64 with recording r's rows permuted to their new numbers) on the device: sdk_diarize_renumber."""
    torch, check, _stream = _native()
    K = tab.K
    _check_tensor("diarize_renumber", "first", first, "int32", (K,))
    _check_tensor("diarize_renumber", "labels", labels, "int32", (tab.C, N_LOCAL))
    _check_tensor("diarize_renumber", "cent64", cent64, "float64", (None, None), K)
    _check_tensor("diarize_renumber", "cent", cent, "float32", tuple(cent64.shape))
    renum = torch.empty((max(K, 1),), dtype=torch.int32, device=labels.device)
    o32, o64 = torch.empty_like(cent), torch.empty_like(cent64)
    check(eng.lib.sdk_diarize_renumber(eng.ctx, first.data_ptr(), tab.cent_off_d.data_ptr(), tab.chunk_off_d.data_ptr(), tab.R, K, tab.C, int(cent.shape[1]),
                                       renum.data_ptr(), labels.data_ptr(), cent.data_ptr(), cent64.data_ptr(), o32.data_ptr(), o64.data_ptr(), _stream()),
          "sdk_diarize_renumber")
    return renum[:K], o32, o64
