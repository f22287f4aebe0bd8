"""Global segment clustering (BASELINE.json config #5; SURVEY.md §8 k5 + k6): spectral clustering of
N L2-normalised embeddings on the rectified cosine affinity, row-sharded over the ranks.

    E_all   = all_gather(E_local)                                  the ONE big exchange (RCCL over xGMI)
    deg     = A 1 ; S = D^-1/2 A D^-1/2                            A = max(E E^T, 0), recomputed per use
    V       = orth(seeded gaussian [N, k])                         CholeskyQR (Gram all-reduce, k x k)
    repeat  : V <- orth(S V)                                       subspace iteration; per step one
                                                                   all-gather of V [N, k] (6.4 MB at 100k x 16)
    Ritz    : H = V^T S V, eigh (k x k, host), U = V Q
    k-means : rows of U normalised; maximin init; Lloyd with centroid all-reduce
    labels  : canonical (order of first appearance over the global row order)

Every O(N^2) and O(N k^2) operation runs in libsdk_hip.so (ops.Engine), and so does the k x k Cholesky + triangular inverse
of every CholeskyQR pass (sdk_chol_inverse, float64): the subspace iteration, the maximin initialisation and the Lloyd passes never
synchronise with the host.  The one k x k eigh of the Ritz step runs on the host in float64, once.  The algorithm is restated for the CPU in
oracle/spectral.py; free choices (rectification, init, iteration counts) are identical.

`provider` is the object that executes the row-block primitives: an ops.Engine on a GPU.  The
distributed control flow itself is device-agnostic, so tests/test_dist_gloo.py drives it on CPU
ranks with an oracle-backed provider.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import dist as sdist
from ._args import THIN_MAX
from .diarize_ops import _check_rows, diarize_centroids
from . import _args
from .ops_cluster import knn_degree, knn_matvec, knn_reverse, knn_rows, knn_rows_fused


@dataclass
class SpectralResult:
    labels: np.ndarray            # [N] int32 canonical, identical on every rank
    eigenvalues: np.ndarray       # [k] descending (of S = D^-1/2 A D^-1/2)
    n_iter: int
    timing: Optional[dict] = None  # seconds per phase when spectral_cluster(..., trace=True) (each phase then ends with a device sync)
    rows: Optional[np.ndarray] = None  # spectral_cluster(..., keep_rows=True): the [N, k] unit rows of the Ritz vectors that k-means clustered (all ranks' rows)
    retried: bool = False          # the subspace iteration was repeated with shifted CholeskyQR (a pivot fell under the relative-pivot rule)


class _Comm:
    def __init__(self, group=None, single: bool = False):
        """single: a whole, unsharded problem on this process alone (nmesc_cluster): off whatever torch.distributed holds, so that nothing
        is all-reduced across ranks that each hold all the rows."""
        import torch.distributed as d
        self.on = not single and d.is_available() and d.is_initialized() and d.get_world_size(group) > 1
        self.group = group
        self.rank = d.get_rank(group) if self.on else 0
        self.world = d.get_world_size(group) if self.on else 1

    def gather_rows(self, local: torch.Tensor, n_total: int) -> torch.Tensor:
        return sdist.all_gather_rows(local, n_total, self.group) if self.on else local

    def sum_(self, x: torch.Tensor) -> torch.Tensor:
        return sdist.all_reduce_sum(x, self.group) if self.on else x


def canonical_labels(lab: np.ndarray) -> np.ndarray:
    lab = np.asarray(lab)
    if lab.size and int(lab.min()) < 0:
        # Engine.kmeans_assign labels a row -1 when its distance to every centre is NaN; remap[-1] would quietly give it the last cluster
        row = int(np.flatnonzero(lab < 0)[0])
        raise ValueError(f"canonical_labels: row {row} has label {int(lab[row])} ({int((lab < 0).sum())} negative in all): k-means labels a row "
                         "-1 when it holds a NaN")
    _, first = np.unique(lab, return_index=True)
    remap = np.full(int(lab.max()) + 1, -1, dtype=np.int32)
    for new, old in enumerate(lab[np.sort(first)]):
        remap[int(old)] = new
    return remap[lab]


def spectral_cluster(provider, E_local: torch.Tensor, Eb_local: torch.Tensor, n_total: int, k: int, n_iter: int = 30,
                     n_kmeans: int = 20, seed: int = 0, group=None, trace: bool = False, keep_rows: bool = False) -> SpectralResult:
    """E_local / Eb_local: this rank's unit-norm embedding rows (fp32 / bf16) under
    dist.shard_bounds(n_total, world).  Returns identical results on every rank."""
    import time
    timing = {} if trace else None
    t_last = [time.perf_counter()]

    def mark(name):
        if trace:
            if Eb_local.is_cuda:
                torch.cuda.synchronize()
            now = time.perf_counter()
            timing[name] = timing.get(name, 0.0) + now - t_last[0]
            t_last[0] = now
    comm = _Comm(group)
    lo, hi = sdist.shard_bounds(n_total, comm.world)[comm.rank]
    n_loc = hi - lo
    dev = Eb_local.device
    assert Eb_local.shape[0] == n_loc, (Eb_local.shape, lo, hi)

    Eb_all = comm.gather_rows(Eb_local.contiguous(), n_total)                      # k5: the embedding all-gather
    ones = torch.ones((n_total, 1), dtype=torch.float32, device=dev)
    deg = provider.affinity_matvec(Eb_all, ones, lo, n_loc)[lo:hi, 0].contiguous()
    dinv_loc = torch.rsqrt(deg)
    dinv_all = comm.gather_rows(dinv_loc.reshape(-1, 1), n_total).reshape(-1).contiguous()
    mark("gather+degrees")

    # seeded start, same gaussian as the oracle (numpy PCG64), orthonormalised across ranks
    G0 = np.random.default_rng(seed).standard_normal((n_total, k))
    V = torch.from_numpy(G0[lo:hi].astype(np.float32)).to(dev)
    # not-positive-definite flag of every CholeskyQR pass (sticky, device side): read once, at the Ritz step's host synchronisation
    spd_flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    V0 = V
    eye = torch.eye(k, dtype=torch.float32, device=dev)

    def apply_S(Vloc: torch.Tensor) -> torch.Tensor:
        Vall = comm.gather_rows(Vloc, n_total)
        Y = provider.affinity_matvec(Eb_all, Vall, lo, n_loc, xscale=dinv_all)[lo:hi].contiguous()
        return provider.rows_apply(Y, eye, scale=dinv_loc)

    def iterate(shifted: bool):
        Vc = _orth(provider, comm, V0, k, spd_flag, shifted)
        mark("init")
        for _ in range(n_iter):
            Y = apply_S(Vc)
            mark("apply_S")
            Vc = _orth(provider, comm, Y, k, spd_flag, shifted)
            mark("orth")
        SVc = apply_S(Vc)
        mark("apply_S")
        return Vc, comm.sum_(provider.rows_gram(Vc, SVc)).double().cpu().numpy()

    retried = False
    V, H = iterate(False)
    flagged = int(comm.sum_(spd_flag.float()).item()) > 0                # every rank takes the same branch (the Gram matrices are all-reduced: normally equal anyway)
    if flagged and np.isfinite(H).all() and hasattr(provider, "set_option"):
        # A pivot fell under the relative-pivot rule (sdk_chol_inverse: cond(Y) > ~1e3): over-clustered or near-duplicate input - lambda_k / lambda_1
        # near 1e-3 - where plain CholeskyQR2 is at the edge of what an fp32 Gram matrix carries.  One retry with SHIFTED CholeskyQR
        # (first pass on G + 1e-5 mean(diag) I, then two plain passes: "CholeskyQR3"), judged by the same rule on its plain passes.
        spd_flag.zero_()
        retried = True
        V, H = iterate(True)
        flagged = int(comm.sum_(spd_flag.float()).item()) > 0
    if flagged or not np.isfinite(H).all():
        # a Gram matrix of the iteration was not positive definite: k exceeds the rank of the embeddings (duplicated rows, fewer
        # distinct segments than clusters) or the input holds NaN.  The host-side CholeskyQR of round 1 raised here too.
        raise np.linalg.LinAlgError(f"spectral_cluster: the k = {k} subspace lost rank (Gram matrix not positive definite): "
                                    "fewer than k independent directions in the embeddings, or non-finite input")
    H = 0.5 * (H + H.T)
    lam, Q = np.linalg.eigh(H)
    order = np.argsort(-lam)
    Qd = torch.from_numpy(np.ascontiguousarray(Q[:, order]).astype(np.float32)).to(dev)
    U = provider.rows_apply(V, Qd)
    R = provider.rows_unit(U)
    mark("ritz")

    labels_loc = _kmeans(provider, comm, R, lo, n_total, k, n_kmeans)
    mark("kmeans")
    lab_all = comm.gather_rows(labels_loc.reshape(-1, 1), n_total).reshape(-1)
    labels = canonical_labels(lab_all.cpu().numpy())
    mark("labels")
    rows = comm.gather_rows(R, n_total).cpu().numpy() if keep_rows else None
    return SpectralResult(labels, lam[order], n_iter, timing, rows, retried)


def _orth(provider, comm: _Comm, Y: torch.Tensor, k: int, spd_flag: Optional[torch.Tensor] = None, shifted: bool = False) -> torch.Tensor:
    """CholeskyQR2: Q = Y R^-1 with R^T R = sum_ranks Y^T Y; applied twice for fp32 stability.  Nothing here synchronises with the
    host: Gram (two-stage, order-fixed) -> all-reduce -> k x k Cholesky + triangular inverse in float64 on the device -> apply.
    shifted: a first pass on G + 1e-5 mean(diag G) I (not judged by the pivot rule), then the two plain passes."""
    if shifted:
        provider.set_option("chol_shift_ppb", 10_000)
        try:
            G = comm.sum_(provider.rows_gram(Y, Y))
            Y = provider.rows_apply(Y, provider.chol_inverse(G, None))
        finally:
            provider.set_option("chol_shift_ppb", 0)
    for _ in range(2):
        G = comm.sum_(provider.rows_gram(Y, Y))
        Y = provider.rows_apply(Y, provider.chol_inverse(G, spd_flag))
    return Y


def _kmeans(provider, comm: _Comm, R: torch.Tensor, lo: int, n_total: int, k: int, n_iter: int) -> torch.Tensor:
    """Maximin initialisation + Lloyd, row-sharded.  Device-side selection throughout (no .item(), no host comparison): at 8 GPUs
    every host round trip would also be a collective everyone waits in.  A row that holds a NaN comes back with label -1
    (Engine.kmeans_assign); nothing here reads the labels on the host, so it is canonical_labels, at the caller's download, that refuses it."""
    dev = R.device
    n_loc = R.shape[0]
    kdim = R.shape[1]

    def fetch_row(grow: torch.Tensor) -> torch.Tensor:
        """The row with this GLOBAL index (0-d int64 tensor on the device), on every rank: the owner contributes it, the others
        zeros; summed."""
        if n_loc:
            loc = (grow - lo).clamp(0, n_loc - 1).reshape(1)
            mine = ((grow >= lo) & (grow < lo + n_loc)).to(torch.float32)
            v = R.index_select(0, loc)[0] * mine
        else:
            v = torch.zeros((kdim,), dtype=torch.float32, device=dev)
        return comm.sum_(v.contiguous())

    def global_argmax(val: torch.Tensor, grow: torch.Tensor) -> torch.Tensor:
        """Global row index of the largest value over the ranks (ties -> lowest row), as a device tensor."""
        if not comm.on:
            return grow
        pair = torch.stack([val.double(), grow.double()])
        out = torch.zeros((comm.world * 2,), dtype=torch.float64, device=dev)
        sdist._gather_into(out, pair, comm.group)
        pairs = out.reshape(comm.world, 2)
        best = pairs[:, 0].max()
        rows = torch.where(pairs[:, 0] == best, pairs[:, 1], torch.full_like(pairs[:, 1], float(n_total)))
        return rows.min().to(torch.int64)

    centres = [fetch_row(torch.zeros((), dtype=torch.int64, device=dev))]
    d2 = torch.empty((max(n_loc, 1),), dtype=torch.float32, device=dev)[:n_loc]
    for j in range(1, k):
        if n_loc:
            provider.kmeans_mindist(R, centres[-1], d2, first=(j == 1))
            val, arg = torch.max(d2, dim=0)                 # first maximum = lowest local row
            grow = arg.to(torch.int64) + lo
        else:
            val = torch.full((), -1.0, dtype=torch.float32, device=dev)
            grow = torch.full((), n_total, dtype=torch.int64, device=dev)
        centres.append(fetch_row(global_argmax(val, grow)))
    C = torch.stack(centres).contiguous()
    # Lloyd: a fixed number of passes.  Once the centres stop moving a pass reproduces them bit for bit (same sums, same counts),
    # so running past convergence changes nothing - and saves the host comparison every pass used to end with.
    for _ in range(n_iter):
        _, _, ps, pc = provider.kmeans_assign(R, C, want_sums=True)
        sums = comm.sum_(ps.double().sum(dim=0))
        cnts = comm.sum_(pc.sum(dim=0).double())
        C = torch.where(cnts[:, None] > 0, sums / cnts.clamp_min(1.0)[:, None], C.double()).float().contiguous()
    labels, _, _, _ = provider.kmeans_assign(R, C, want_sums=False)
    return labels


# ------------------------------------------------------------------ k6, threshold path: centroid-linkage agglomerative clustering
PYANNOTE_THRESHOLD = 0.7045654963945799        # PyAnnote 3.1's published default for ITS trained ResNet34 embedding
PYANNOTE_MIN_CLUSTER_SIZE = 12


@dataclass
class AgglomerativeResult:
    labels: np.ndarray            # [N] int32 canonical (order of first appearance)
    linkage: np.ndarray           # [N - 1, 4] float64, scipy's layout and numbering (Engine.centroid_linkage)
    n_large: int                  # clusters at least the effective minimum size after the cut (all clusters when n_clusters is given)
    forced = None                 # speakers= overruled the cut: {found, target, method: "level", level, n_iter: None} (a class default, not a field)


def _flat_partition(Z: np.ndarray, n: int, n_merges: int) -> np.ndarray:
    """Canonical labels of the partition formed by the first n_merges rows of Z (union-find over node ids)."""
    parent = np.arange(2 * n - 1 if n > 0 else 0, dtype=np.int64)

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r
    for t in range(n_merges):
        a, b = int(Z[t, 0]), int(Z[t, 1])
        parent[find(a)] = n + t
        parent[find(b)] = n + t
    if n == 0:
        return np.zeros(0, np.int32)
    roots = np.array([find(i) for i in range(n)], dtype=np.int64)
    return canonical_labels(roots).astype(np.int32)


def cut_level(Z: np.ndarray, t: float) -> int:
    """The number of merges that fcluster_distance(Z, t) keeps: the rows of Z before the first whose height exceeds t."""
    Z = np.asarray(Z, dtype=np.float64)
    above = np.flatnonzero(Z[:, 2] > t)
    return int(above[0]) if above.size else int(Z.shape[0])


def fcluster_distance(Z: np.ndarray, t: float) -> np.ndarray:
    """The flat cut of linkage Z at distance t: canonical labels of the partition formed by the merges BEFORE the first row whose height
    exceeds t (numpy only).

    For a linkage made by repeated global-minimum merges (Engine.centroid_linkage, scipy's centroid linkage) this equals
    scipy.cluster.hierarchy.fcluster(Z, t, "distance") even with inversions (non-monotone heights).  Let row k be the first with height > t.
      - Every earlier merge is <= t: each cluster formed by rows 0 .. k-1 has no height above t inside it, so the cut keeps it whole.
      - At step k every live pair is > t: row k was the global minimum over the clusters alive then.
      - Every later node contains a merge above t: following it down, the first merge made at step >= k joined clusters alive at step k
        (or nodes made of them), at a height > t.  So no later node is kept whole, and no two of the step-k clusters are joined.
    """
    Z = np.asarray(Z, dtype=np.float64)
    n = Z.shape[0] + 1
    return _flat_partition(Z, n, cut_level(Z, t))


# ------------------------------------------------------------------ linked centroid linkage: rows that must stay apart (speakers across recordings)
@dataclass
class LinkResult:
    labels: np.ndarray            # [N] int32 canonical (order of first appearance)
    linkage: np.ndarray           # [N - 1, 4] float64: the merges made, in scipy's layout and numbering; the rows from n_merges on are zero
    n_merges: int


def link_rows(provider, E, group, threshold: float) -> LinkResult:
    """Clusters of the unit rows E ([N, d] fp32 on the provider's device) in which no two rows of one group meet: the linked centroid linkage
    (Engine.linked_linkage, sdk_linked_linkage; the rule heads csrc/ahc.hip) run with stop = threshold, so the device makes only the merges at
    or below it.  group [N] ints: rows with the same group >= 0 are forbidden to each other, and so are clusters that hold such rows; a negative
    group is a free row.  labels = _flat_partition(Z, N, n_merges), canonical.  Parity with any outside tool is unpinned: the tests pin this rule.
    N == 0 and N == 1 are answered on the host."""
    N = int(E.shape[0])
    if N <= 1:
        return LinkResult(np.zeros(N, np.int32), np.zeros((0, 4)), 0)
    g = np.ascontiguousarray(group.detach().cpu().numpy() if isinstance(group, torch.Tensor) else group).astype(np.int32)
    if g.shape != (N,):
        raise ValueError(f"link_rows: group must be [N] = [{N}], got {list(g.shape)}")
    if not float(threshold) >= 0.0:
        raise ValueError(f"link_rows: threshold={threshold} (a distance >= 0)")
    gd = torch.from_numpy(g).to(E.device) if isinstance(E, torch.Tensor) else g
    Z, merges = provider.linked_linkage(E, gd, None, float(threshold))
    Z = Z.cpu().numpy()
    m = int(merges.cpu().numpy()[0])
    return LinkResult(_flat_partition(Z, N, m), Z, m)


# ------------------------------------------------------------------ bounds on the speaker count (`speakers=`)
# bounds      (this build's statement of pyannote's num_speakers / min_speakers / max_speakers, written from the published description; no
#             pyannote code is on hand: PARITY IS UNPINNED, the tests pin THIS rule).  speakers = None: no bound, today's path.  An int k >= 1:
#             exactly k (lo = hi = k).  A pair (lo, hi), either side None, 1 <= lo <= hi: bounds.  pyannote's max_speakers is
#             speakers=(None, hi) here; Diarizer.run's max_speakers is the cap PER FRAME and never touches the clustering.
#               1. the unbounded clustering runs first and finds K0 speakers ("ahc": the clusters after cut and fold; "vbx": the kept ones);
#               2. lo <= K0 <= hi: the result IS the unbounded one, bit for bit;
#               3. otherwise target = lo when K0 < lo, else hi, clamped to 1 .. N (N training rows);
#               4. fewer than two training rows: nothing is forced;
#               5. "ahc": the level search of agglomerative_cluster; "vbx": kmeans_cluster with k = target on the original unit rows.
def parse_speakers(speakers, who: str = "speakers"):
    """speakers (None, an int k >= 1, or a pair (lo, hi) with either side None and 1 <= lo <= hi) -> None or (lo, hi) with hi = None for no
    upper bound.  Anything else is a ValueError; nothing here touches the device."""
    def one(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{who}: speakers={speakers!r} (None, an int k >= 1, or a pair (lo, hi) of ints or None with 1 <= lo <= hi)")
        return int(v)
    if speakers is None:
        return None
    if isinstance(speakers, (tuple, list)):
        if len(speakers) != 2:
            one(None)
        lo, hi = (None if v is None else one(v) for v in speakers)
    else:
        lo = hi = one(speakers)
    lo = 1 if lo is None else lo
    if lo < 1 or (hi is not None and hi < lo):
        one(None)
    return lo, hi


def speaker_target(found: int, bounds, n_rows: int) -> Optional[int]:
    """Rules 2 - 4 of the bounds: None when the count found stands, else the count to force."""
    if bounds is None or n_rows < 2:
        return None
    lo, hi = bounds
    if found >= lo and (hi is None or found <= hi):
        return None
    return min(max(lo if found < lo else hi, 1), int(n_rows))


def level_counts(Z: np.ndarray, eff: int) -> np.ndarray:
    """L [N] int64: L[t] = the clusters of at least eff rows after the first t merges of the linkage Z [N - 1, 4], in ONE pass over Z's sizes:
    merge t joins nodes a and b (a leaf has one row, node N + i has Z[i, 3]) into one of Z[t, 3] rows, so
    L[t + 1] = L[t] + [Z[t, 3] >= eff] - [size a >= eff] - [size b >= eff]."""
    Z = np.asarray(Z, dtype=np.float64)
    N = Z.shape[0] + 1
    size = np.concatenate([np.ones(N, np.int64), np.rint(Z[:, 3]).astype(np.int64)])
    big = (size >= int(eff)).astype(np.int64)
    step = big[N:] - big[Z[:, 0].astype(np.int64)] - big[Z[:, 1].astype(np.int64)]
    return np.concatenate([[N * int(big[0])], N * int(big[0]) + np.cumsum(step)]).astype(np.int64)


def level_search(Z: np.ndarray, eff: int, t0: int, target: int):
    """The level of the forced count: the t in 0 .. N - 1 that minimises (|L[t] - target|, |t - t0|, t) -> (t, L[t])."""
    L = level_counts(Z, eff)
    t = np.arange(L.size)
    best = np.lexsort((t, np.abs(t - int(t0)), np.abs(L - int(target))))[0]
    return int(best), int(L[best])


def agglomerative_cluster(provider, E, threshold: float = PYANNOTE_THRESHOLD, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
                          n_clusters: Optional[int] = None, speakers=None) -> AgglomerativeResult:
    """Speaker clusters without knowing their number: centroid linkage on the unit rows E ([N, d] fp32 on the provider's device; the linkage
    runs in libsdk_hip.so, Engine.centroid_linkage), a flat cut at `threshold`, small clusters folded into the nearest large one.

    This restates the threshold path of PyAnnote 3.1's AgglomerativeClustering as stated here (written from its published description, not
    from its code; the tests pin THIS rule):
      1. the effective minimum size is min(min_cluster_size, max(1, round(0.1 N)))  (Python's round: half to even);
      2. clusters of the cut with at least that many rows are large;
      3. no large cluster: every label is 0;
      4. otherwise every small cluster joins the large cluster whose centroid (mean of its unit rows) is nearest in 1 - cos, ties to the
         large cluster that comes first in label order;
      5. N == 1 gives [0];
      6. n_clusters given: the partition after the first N - n_clusters merges, min_cluster_size not applied.  For a count that respects
         the minimum size, pass `speakers` (rule 7).
      7. speakers given (parse_speakers; the bounds stated above it; PyAnnote's search over dendrogram levels, written from the published
         description, parity unpinned, the tests pin THIS rule): rules 1 - 5 run first and find K0 clusters (n_large, or 1 when no
         cluster is large).  Inside the bounds the result is that one.  Otherwise, with target from speaker_target, eff from rule 1 and
         t0 = the merges the cut keeps (cut_level), let L(t) be the clusters of at least eff rows after the first t merges, t = 0 .. N - 1
         (level_counts: host integers on Z's size column, O(N)).  The level t* minimises (|L(t) - target|, |t - t0|, t); the partition
         after t* merges is folded by rules 2 - 4 as the cut is.  Every target <= K0 is reached: a merge changes L by +1, 0 or -1, so L
         moves in unit steps from L(t0) = K0 (wherever a cluster is large) down to L(N - 1) = 1.  A target > K0 may be out of
         reach when eff > 1 (fewer than target clusters of eff rows at any level): the closest count is taken.  The result's `forced`
         then says what was found and what was taken.
    Labels are canonical (order of first appearance)."""
    bounds = parse_speakers(speakers, "agglomerative_cluster")
    if bounds is not None and n_clusters is not None:
        raise ValueError("agglomerative_cluster: n_clusters and speakers are two ways to a count: pass one")
    N = int(E.shape[0])
    if N == 0:
        return AgglomerativeResult(np.zeros(0, np.int32), np.zeros((0, 4)), 0)
    Z = provider.centroid_linkage(E).cpu().numpy() if N > 1 else np.zeros((0, 4))
    if N == 1:
        return AgglomerativeResult(np.zeros(1, np.int32), Z, 1)
    if n_clusters is not None:
        k = min(max(int(n_clusters), 1), N)
        lab = _flat_partition(Z, N, N - k)
        return AgglomerativeResult(lab, Z, int(lab.max()) + 1)
    Eh = E.detach().cpu().numpy().astype(np.float64) if isinstance(E, torch.Tensor) else np.asarray(E, dtype=np.float64)
    lab, n_large = fold_small_clusters(Eh, fcluster_distance(Z, threshold), min_cluster_size)
    res = AgglomerativeResult(lab, Z, n_large)
    target = speaker_target(max(n_large, 1), bounds, N)
    if target is not None:
        level, _ = level_search(Z, effective_min_size(min_cluster_size, N), cut_level(Z, threshold), target)
        res.labels, res.n_large = fold_small_clusters(Eh, _flat_partition(Z, N, level), min_cluster_size)
        res.forced = {"found": max(n_large, 1), "target": target, "method": "level", "level": level, "n_iter": None}
    return res


def effective_min_size(min_cluster_size: int, N: int) -> int:
    """Rule 1 of agglomerative_cluster."""
    return min(int(min_cluster_size), max(1, round(0.1 * N)))


def fold_small_clusters(E: np.ndarray, labels: np.ndarray, min_cluster_size: int):
    """Rules 1-4 of agglomerative_cluster on a flat partition (canonical labels) of the rows E (float64): -> (canonical labels, large count)."""
    N = labels.shape[0]
    eff = effective_min_size(min_cluster_size, N)
    K = int(labels.max()) + 1
    sizes = np.bincount(labels, minlength=K)
    large = np.flatnonzero(sizes >= eff)
    if large.size == 0:
        return np.zeros(N, np.int32), 0
    if large.size == K:
        return canonical_labels(labels).astype(np.int32), K
    cent = np.zeros((K, E.shape[1]))
    np.add.at(cent, labels, E)
    cent /= sizes[:, None]
    unit = cent / np.linalg.norm(cent, axis=1, keepdims=True).clip(1e-300)
    small = np.flatnonzero(sizes < eff)
    dist = 1.0 - unit[small] @ unit[large].T          # [small, large] cosine distance
    to = large[np.argmin(dist, axis=1)]                # first minimum: the large cluster first in label order
    remap = np.arange(K)
    remap[small] = to
    return canonical_labels(remap[labels]).astype(np.int32), int(large.size)


# ------------------------------------------------------------------ VBx: the linkage only initialises a variational-Bayes mixture in PLDA space
VBX_AHC_THRESHOLD = 0.6          # the initial cut of the linkage (an over-split is what the mixture repairs)
VBX_FA, VBX_FB, VBX_MAX_ITERS, VBX_EPSILON, VBX_INIT_SMOOTHING = 0.07, 0.8, 20, 1e-4, 7.0
VBX_MIN_PI = 1e-7                # speakers whose weight falls to this or below have died out (the kernel's constant)
VBX_LOOP_PROB = 0.99             # BUT's value for THEIR x-vectors at a 0.25-s step; unpinned here (no trained model on hand to tune it on)


@dataclass
class VbxResult:
    labels: np.ndarray            # [N] int32: the arg-max of gamma over the kept speakers (ties to the lower); reported, not used for assignment
    n_speakers: int               # K, the speakers with pi > 1e-7
    pi: np.ndarray                # [S] float64 speaker weights after the last iteration
    elbo: np.ndarray              # [n_iter] float64
    n_iter: int
    keep: np.ndarray              # [K] int32: the kept speakers among the S initial clusters, ascending
    init_labels: np.ndarray       # [N] int32 canonical labels of the initial cut (S = max + 1 clusters)
    cent: object                  # [K, d] fp32 unit centroids (device tensor)
    cent64: object                # [K, d] float64, the same before the final rounding (device tensor; what sdk_diarize_assign reads)
    gamma: object                 # [N, S] float64 responsibilities (device tensor)
    # speakers= overruled the mixture: {found, target, method: "kmeans", level: None, n_iter}; labels, n_speakers, cent and cent64 are then
    # kmeans_cluster's, and pi, elbo, n_iter, keep, init_labels and gamma stay those of the VBx pass that was overruled (a class default, not a field)
    forced = None


def vbx_cluster(provider, E, plda, threshold: float = VBX_AHC_THRESHOLD, Fa: float = VBX_FA, Fb: float = VBX_FB, max_iters: int = VBX_MAX_ITERS,
                epsilon: float = VBX_EPSILON, init_smoothing: float = VBX_INIT_SMOOTHING, rows=None, speakers=None,
                loop_prob: float = 0.0) -> VbxResult:
    """VBx clustering (Landini et al., BUT) of the unit rows E ([R, d] fp32 on the provider's device; rows: the ascending row numbers that
    take part, host integers, None = all), as the clustering half of PyAnnote's speaker-diarization-community-1 pipeline is stated HERE
    (written from the published description; no trained PLDA and no pyannote code is on hand: PARITY IS UNPINNED, the tests pin this rule):

      transform       x = the PLDA transform of every row (plda.py), float64, on the device (sdk_plda_transform)
      initialisation  Engine.centroid_linkage on the rows, cut with fcluster_distance(Z, threshold), no small-cluster fold: S canonical
                      clusters; gamma0[t, s] = softmax_s(init_smoothing [label_t == s]); pi = 1 / S
      iteration       float64; without the HMM at loop_prob = 0 (the embeddings of overlapping chunks are not a chain; HMM below).  With
                      rho = x sqrt(Phi), G_t = -(|x_t|^2 + D ln 2 pi) / 2, for ii = 0 .. max_iters - 1:
                        N_s = sum_t gamma[t, s];  invL[s, :] = 1 / (1 + (Fa / Fb) N_s Phi);  alpha[s, :] = (Fa / Fb) invL[s, :] sum_t gamma[t, s] rho[t, :]
                        logp[t, s] = Fa (rho_t . alpha_s - sum_d (invL[s, d] + alpha[s, d]^2) Phi_d / 2 + G_t)
                        z = logp + ln pi (pi_s == 0: -inf, and gamma[:, s] is exactly 0 from then on);  lse_t = logsumexp_s z[t, :] with the
                        maximum subtracted;  gamma = exp(z - lse)
                        ELBO = sum_t lse_t + (Fb / 2) sum_{s, d} (ln invL - invL - alpha^2 + 1);  pi = sum_t gamma / sum_{t, s} gamma
                        stop after this iteration when ii > 0 and ELBO - ELBO_prev < epsilon
                      All iterations are enqueued at once (sdk_vbx); the stop test runs on the device.
      HMM             loop_prob = P in (0, 1) (default 0: the iteration above, unchanged): VBx as published, a Bayesian HMM over a sequence.
                      THE ROWS MUST THEN BE IN TIME ORDER (the windows of Backend.cluster_ranges are; the (chunk, local speaker) rows of
                      Diarizer.run are not a chain, and it passes no loop_prob).  The speaker of row t is the speaker of row t - 1 with
                      probability P, else drawn from pi: tr[i][j] = P [i == j] + (1 - P) pi_j, never formed.  logp, invL, alpha, the
                      ELBO's second term, the stop test and the first iteration's pi = 1 / S are as above; z, lse and gamma become, in the
                      log domain (ln(1 - P) = log1p(-P); logaddexp(a, b) = max + log1p(exp(min - max)): an argument of -inf returns the
                      other exactly; every logsumexp with the maximum subtracted):
                        lf[0, s] = logp[0, s] + ln pi_s;  m_t = logsumexp_s lf[t, s]
                        lf[t, s] = logp[t, s] + logaddexp(ln P + lf[t-1, s], (ln(1 - P) + ln pi_s) + m_{t-1})                    t >= 1
                        lb[n-1, s] = 0;  q_s = logp[t+1, s] + lb[t+1, s];  r = logsumexp_s(ln pi_s + q_s)
                        lb[t, s] = logaddexp(ln P + q_s, ln(1 - P) + r)                                                          t < n - 1
                        tll = m_{n-1};  gamma[t, s] = exp(lf[t, s] + lb[t, s] - tll);  ELBO = tll + (Fb / 2) sum_{s, d} (...)
                        pi'_s = gamma[0, s] + ((1 - P) pi_s) sum_{t >= 1} exp(m_{t-1} + logp[t, s] + lb[t, s] - tll);  pi = pi' / sum_s pi'_s
                      (sdk_vbx_hmm: both passes in one launch, a step is two cross-lane reductions; csrc/vbx.hip).  VBX_LOOP_PROB (0.99) is
                      BUT's value for their x-vectors at a 0.25-s step; like the rest of VBx it is unpinned here.
      result          speakers with pi > 1e-7 are kept, in their order; a kept speaker's centroid is sum_t gamma[t, k] e_t / sum_t gamma[t, k]
                      over the ORIGINAL unit rows, summed in float64 in ascending row order, re-normalised (sdk_vbx_centroids); a row's hard
                      label is the arg-max of gamma over the kept speakers, ties to the lower.
      bounds          speakers given (parse_speakers; the bounds stated above it; community-1's fallback as best known here, written from the
                      published description, parity unpinned, the tests pin THIS rule): the pass above runs first and keeps K0 speakers.
                      Inside the bounds the result is that one.  Otherwise kmeans_cluster with k = target (speaker_target; above
                      KMEANS_MAX_K it is a ValueError) on the original unit rows gives labels, n_speakers, cent and cent64; pi, elbo and
                      the rest stay those of the pass that was overruled, and `forced` says what was found and what was taken.

    Needs at least two rows.  The linkage Z is downloaded for the cut; after that one host read decides (n_iter, status, K, at the end; a
    non-finite row raises ValueError there), and the results (labels, pi, elbo, keep) are downloaded after it."""
    loop_prob = float(loop_prob)
    if not 0.0 <= loop_prob < 1.0:
        raise ValueError(f"vbx_cluster: loop_prob={loop_prob} (at least 0, below 1)")                  # a NaN fails both
    bounds = parse_speakers(speakers, "vbx_cluster")
    R = int(E.shape[0])
    rows_h = np.arange(R, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    N = int(rows_h.size)
    if N < 2:
        raise ValueError(f"vbx_cluster: {N} rows (VBx needs at least 2)")
    if rows_h.min() < 0 or rows_h.max() >= R or (np.diff(rows_h) <= 0).any():
        raise ValueError(f"vbx_cluster: rows must ascend strictly inside [0, {R}), got {int(rows_h.min())} .. {int(rows_h.max())}")
    rows_d = torch.from_numpy(rows_h.astype(np.int32)).to(E.device)
    Et = E if rows is None else E.index_select(0, rows_d.long()).contiguous()
    Z = provider.centroid_linkage(Et).cpu().numpy()
    init = fcluster_distance(Z, threshold).astype(np.int32)
    S = int(init.max()) + 1
    X = provider.plda_transform(E, rows_d, plda, check_rows=False)
    if loop_prob == 0.0:
        gamma, pi, elbo, n_iter, status = provider.vbx(X, plda.device_arrays(E.device)["Phi"], torch.from_numpy(init).to(E.device), S, Fa, Fb, max_iters,
                                                       epsilon, init_smoothing)
    else:
        gamma, pi, elbo, n_iter, status = provider.vbx_hmm(X, plda.device_arrays(E.device)["Phi"], torch.from_numpy(init).to(E.device), S, loop_prob,
                                                           Fa, Fb, max_iters, epsilon, init_smoothing)
    K, keep, labels, cent, cent64 = provider.vbx_centroids(gamma, pi, E, rows_d, check_rows=False)
    n_it, st, Kn = (int(v) for v in torch.cat([n_iter, status, K]).cpu().numpy())       # the one read
    if st:
        raise ValueError(f"vbx_cluster: non-finite input (status {st}: 1 = a non-finite embedding or PLDA value, 4 = a non-finite ELBO after "
                         f"{n_it} iterations)")
    res = VbxResult(labels.cpu().numpy(), Kn, pi.cpu().numpy(), elbo[:n_it].cpu().numpy(), n_it, keep[:Kn].cpu().numpy(), init, cent[:Kn], cent64[:Kn],
                    gamma)
    target = speaker_target(Kn, bounds, N)
    if target is not None:
        if target > KMEANS_MAX_K:
            raise ValueError(f"vbx_cluster: speakers={speakers!r} asks for {target} speakers ({Kn} found); the k-means serves at most {KMEANS_MAX_K}")
        km = kmeans_cluster(provider, E, target, rows=rows_h)
        res.labels, res.n_speakers, res.cent, res.cent64 = km.labels, km.n_clusters, km.cent, km.cent64
        res.forced = {"found": Kn, "target": target, "method": "kmeans", "level": None, "n_iter": km.n_iter}
    return res


# ------------------------------------------------------------------ spherical k-means on unit rows: the forced count of "vbx"
KMEANS_MAX_K = 64                # one lane per centre (csrc/kmeans.hip)
KMEANS_MAX_ITERS = 20
KMEANS_MAX_ROWS = 65536
KMEANS_SEGMENT = 1024            # rows per segment of the centre sums (the kernel's constant)
KMEANS_HOST_READS = 2            # kmeans_cluster waits for the device twice: the one read (n_iter, status), then the labels


@dataclass
class KmeansResult:
    labels: np.ndarray            # [N] int32 canonical (order of first appearance), centres left without rows dropped
    n_clusters: int               # K <= k
    n_iter: int                   # assignments made
    cent: object                  # [K, d] fp32 unit centroids of the labels (device tensor; sdk_diarize_centroids)
    cent64: object                # [K, d] float64, the same before the final rounding (device tensor; what sdk_diarize_assign reads)
    counts: np.ndarray            # [K] int64 rows per cluster


def kmeans_cluster(provider, E, k: int, rows=None, max_iters: int = KMEANS_MAX_ITERS) -> KmeansResult:
    """Spherical k-means with k centres on the unit rows E, on the device with the whole loop in one enqueue (Engine.kmeans_rows,
    sdk_kmeans_rows; csrc/kmeans.hip).  The rule (this build's; the tests pin it; row t below is E[rows[t]]):

      input       E [R, d] fp32 unit rows on the provider's device, d = 64, 128, .. 512 (the widths sdk_diarize_assign serves); rows: the
                  ascending row numbers that take part, strictly inside [0, R), host integers (None = all), N = len(rows) <= 65 536;
                  1 <= k <= min(N, KMEANS_MAX_K = 64); 1 <= max_iters <= 1000.  Anything else is a ValueError before the launch.
      seeding     maximin, as the thin k-means of spectral_cluster: centre 0 is row 0; centre j is the row whose largest cosine to the
                  centres 0 .. j - 1 is smallest, ties to the lowest row.  Seeds are rows, so their cosines are sums of exact products,
                  added in float64 over the columns in ascending order.
      assignment  label_t = argmax_c <centre c, row t>: each cosine one float64 sum over the columns in ascending order (an fma chain);
                  ties to the lower c; a NaN never wins.
      update      s_c = the float64 sum of the rows labelled c, in this order: per segment of KMEANS_SEGMENT = 1024 rows (t = 1024 g ..
                  1024 g + 1023) in ascending row order from 0.0, then the segments' partials in segment order from 0.0; centre c =
                  s_c / |s_c|.  A centre without rows, or with |s_c| = 0, keeps its value.  No atomics.
      stop        iteration it = 0, 1, ..: assignment, then update.  The loop stops after the first assignment with it >= 1 in which
                  no label changed, or after max_iters assignments; n_iter counts the assignments made.  All iterations are enqueued
                  at once; the stop flag lives on the device and later launches return on it, as in sdk_vbx.  ONE host read at the end,
                  (n_iter, status); status != 0 (a non-finite value in a row) raises ValueError after that read.
      result      the labels of the last assignment, downloaded after the read; centres left without rows are dropped and the labels
                  made canonical; cent / cent64 come from sdk_diarize_centroids over those labels (the float64 mean of the unit rows in
                  ascending row order, re-normalised), in the layout sdk_diarize_assign takes."""
    import torch as _torch
    _check_rows("kmeans_cluster", E)
    R = int(E.shape[0])
    rows_h = np.arange(R, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    N = int(rows_h.size)
    if N < 1 or N > KMEANS_MAX_ROWS:
        raise ValueError(f"kmeans_cluster: {N} rows (1 .. {KMEANS_MAX_ROWS})")
    if rows_h.min() < 0 or rows_h.max() >= R or (np.diff(rows_h) <= 0).any():
        raise ValueError(f"kmeans_cluster: rows must ascend strictly inside [0, {R}), got {int(rows_h.min())} .. {int(rows_h.max())}")
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1 or k > min(N, KMEANS_MAX_K):
        raise ValueError(f"kmeans_cluster: k={k!r} (an int, 1 .. min(N, {KMEANS_MAX_K}), N={N})")
    max_iters = int(max_iters)
    if max_iters < 1 or max_iters > 1000:
        raise ValueError(f"kmeans_cluster: max_iters={max_iters} (1 .. 1000)")
    rows_d = _torch.from_numpy(rows_h.astype(np.int32)).to(E.device)
    lab_d, n_iter, status = provider.kmeans_rows(E, rows_d, int(k), max_iters, check_rows=False)
    n_it, st = (int(v) for v in _torch.cat([n_iter, status]).cpu().numpy())                # the one read
    if st:
        raise ValueError(f"kmeans_cluster: non-finite input (status {st}: a row holds a NaN or an infinity)")
    labels = canonical_labels(lab_d.cpu().numpy()).astype(np.int32)
    K = int(labels.max()) + 1
    cent, cent64 = diarize_centroids(provider, E, rows_d, _torch.from_numpy(labels).to(E.device), K, check_rows=False)
    return KmeansResult(labels, K, n_it, cent, cent64, np.bincount(labels, minlength=K).astype(np.int64))


# ------------------------------------------------------------------ NME-SC: spectral clustering on a pruned nearest-neighbour graph, no threshold
# nmesc       (clustering="nmesc"; the eigengap spectral clustering with normalised-maximum-eigengap pruning that NeMo's diarizer defaults to,
#             written from the published description; no NeMo code is on hand: PARITY IS UNPINNED, the tests pin THIS rule).  The input is
#             the n training rows X of one recording: unit rows, fp32 [n, d], d a width the row kernels serve, 2 <= n <= 65 536.
#   cosine      c(i, j) = the float64 sum, in ascending column order, of the exact products x_i[t] x_j[t] (diarize_host._dot_in_order's
#               arithmetic): symmetric bit for bit.  A row with a non-finite value is a ValueError that names it.
#   lists       P = min(NMESC_P_MAX = 64, n - 1).  Row i's list: the P rows j != i of largest c(i, j), ties to the lower j, in that order:
#               idx int32 [n, P], cos float64 [n, P] (sdk_knn_rows).
#   graph       at p <= P: B_p(i, j) = 1 iff j is among the first p entries of list i; A_p = B_p + B_p^T (entries 0, 1, 2);
#               deg_p(i) = p + in_p(i), integers; T_p = (I + D^-1/2 A_p D^-1/2) / 2.  The lazy form is the point: a nearest-neighbour
#               graph has eigenvalues near -1 (p = 1 gives matched pairs), to which plain subspace iteration on D^-1/2 A D^-1/2 would
#               converge; T_p's spectrum lies in [0, 1] in the same order.
#   candidates  the members of NMESC_NEIGHBOURS = (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64) that are <= P; none: the one candidate (P,).
#               `neighbours` replaces NMESC_NEIGHBOURS.
#   spectrum    per candidate p the m = min(n, max_count + 1) largest eigenvalues tau_1 >= .. >= tau_m of T_p, block width
#               b = min(n, THIN_MAX, m + 8).  n <= NMESC_DENSE_ROWS = 64: on the host, the dense T_p built from the downloaded lists,
#               numpy.linalg.eigh in float64.  Above: on the device, from the seeded gaussian [n, b] (numpy default_rng(seed)), n_iter
#               steps of V <- orth(T_p V) (CholeskyQR2, _orth; sdk_knn_matvec), the Ritz step H = V^T T_p V with sdk_sym_eigh, the first m
#               values.  All candidates' eigenvalues come down in ONE download.
#   selection   nmesc_select, host float64 on that table: g_i(p) = tau_i - tau_{i+1} for i in [lo, hi], the bounds of `speakers`
#               (parse_speakers) clipped to 1 .. m - 1, default 1 .. m - 1; k(p) = the lowest i of largest g_i(p), g(p) that gap;
#               r(p) = p / g(p), +inf when g(p) <= NMESC_FLAT_GAP = 1e-6; p* = the candidate of least r, ties to the lower p; k* = k(p*).
#               Every r infinite: k* = lo, p* = the largest candidate.  The bounds are part of the rule: nothing is `forced`.
#   labels      k* = 1: every label 0.  Otherwise the first k* Ritz vectors of T_p* (same seed and block; the host's eigenvectors for
#               n <= NMESC_DENSE_ROWS) go through rows_unit and the maximin + Lloyd k-means of spectral_cluster (_kmeans) with
#               NMESC_KMEANS_PASSES = 20 passes, then canonical_labels.
# multi-scale (nmesc_multiscale; the method was published with it: Park et al., "Multi-scale speaker diarization with neural affinity score
#             fusion", ICASSP 2021, as NeMo's clustering diarizer runs it, with FIXED weights here: nothing is learned or tuned).  Every
#             stretch of speech is embedded at S window lengths, longest first, the shortest being the BASE scale (wav.scale_starts states
#             the windows and the map).  E_all fp32 [n_all, d] stacks the unit rows of every scale, maps int32 [S, n] names for base window i
#             its row maps[s][i] of E_all at scale s (the window of that scale whose centre is nearest).
#   weights     None: 1 / S each.  Given: S numbers, finite, >= 0, not all zero, divided by their sum in float64 on the host; that array
#               is what the kernel and the restatement both receive.
#   fused       for base windows i != j: c_s(i, j) = `cosine` above of the rows maps[s][i] and maps[s][j];
#               f(i, j) = (..((0 + w_0 c_0) + w_1 c_1) .. + w_{S-1} c_{S-1}), float64, every product and every sum rounded once.  A NaN f
#               ranks as -inf.  Symmetric bit for bit, as c_s is.
#   lists       as above with f in place of c (sdk_knn_rows_fused, knn_rows_fused_host).  A map entry that is not a row of E_all, or a
#               non-finite row that a map names, is a ValueError; a non-finite row no map names is not looked at.
#   the rest    graph, candidates, spectrum, selection and labels are the rule above on those lists, unchanged: nothing behind the lists
#               reads the rows.  With S = 1 and the identity map the whole result is nmesc_cluster's.
NMESC_P_MAX = 64
NMESC_NEIGHBOURS = (2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)
NMESC_DENSE_ROWS = 64
NMESC_MAX_COUNT = 15
NMESC_N_ITER = 30
NMESC_KMEANS_PASSES = 20
NMESC_FLAT_GAP = 1e-6
NMESC_MAX_ROWS = 65536


@dataclass
class NmescResult:
    labels: np.ndarray            # [n] int32 canonical
    n_speakers: int               # k*
    p: int                        # p*, the neighbours kept
    ps: tuple                     # the candidates
    eigenvalues: np.ndarray       # [n_p, m] float64, descending per candidate
    ratios: np.ndarray            # [n_p] float64 r(p), +inf for a flat spectrum
    n_iter: int                   # steps of the subspace iteration (0: the host's dense eigensolve)
    retried: bool = False         # the sweep was repeated with shifted CholeskyQR (spectral_cluster's rule)
    host_reads: int = 0           # the waits for the device this call made
    scales: int = 1               # the scales whose affinities were fused (nmesc_multiscale; 1: the one table of nmesc_cluster)


def nmesc_candidates(n: int, neighbours=None) -> tuple:
    """The candidates of the rule for n >= 2 rows."""
    P = min(NMESC_P_MAX, int(n) - 1)
    src = NMESC_NEIGHBOURS if neighbours is None else tuple(neighbours)
    if not src or any(isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, np.integer)) or p < 1 for p in src):
        raise ValueError(f"nmesc: neighbours={neighbours!r} (a sequence of ints >= 1)")
    ps = tuple(sorted({int(p) for p in src if p <= P}))
    return ps if ps else (P,)


def _nmesc_shape(n: int, max_count):
    """-> (m, b) of the rule."""
    if isinstance(max_count, (bool, np.bool_)) or not isinstance(max_count, (int, np.integer)) or not 1 <= max_count <= THIN_MAX - 1:
        raise ValueError(f"nmesc: max_count={max_count!r} (an int, 1 .. {THIN_MAX - 1})")
    m = min(int(n), int(max_count) + 1)
    return m, min(int(n), THIN_MAX, m + 8)


def nmesc_select(ps, taus, bounds, n: int):
    """The selection of the rule, a pure function: ps the candidates (ascending), taus [n_p, m] float64 their eigenvalues in descending order,
    bounds None or parse_speakers' (lo, hi), n the rows -> (p*, k*, ratios [n_p] float64, ks [n_p] int)."""
    taus = np.asarray(taus, dtype=np.float64)
    ps = [int(p) for p in ps]
    if taus.ndim != 2 or taus.shape[0] != len(ps) or not ps or taus.shape[1] < 2 or taus.shape[1] > int(n):
        raise ValueError(f"nmesc_select: taus must be [{len(ps)}, m] with 2 <= m <= n = {n}, got {list(taus.shape)}")
    if not np.isfinite(taus).all():
        raise ValueError("nmesc_select: a non-finite eigenvalue")
    m = taus.shape[1]
    lo, hi = (1, None) if bounds is None else bounds
    hi = m - 1 if hi is None else min(int(hi), m - 1)
    lo = min(max(int(lo), 1), m - 1)
    hi = max(hi, lo)
    gaps = taus[:, lo - 1:hi] - taus[:, lo:hi + 1]                   # column c is g_{lo + c}
    at = np.argmax(gaps, axis=1)                                    # first maximum: the lowest i
    ks = (lo + at).astype(np.int64)
    g = gaps[np.arange(len(ps)), at]
    ratios = np.where(g > NMESC_FLAT_GAP, np.asarray(ps, np.float64) / np.where(g > NMESC_FLAT_GAP, g, 1.0), np.inf)
    if not np.isfinite(ratios).any():
        return ps[-1], lo, ratios, ks
    best = int(np.argmin(ratios))                                   # first minimum: ps ascend, so the lower p
    return ps[best], int(ks[best]), ratios, ks


# ---- the graph in numpy (what the kernels of csrc/nmesc.hip compute, bit for bit)
def knn_rows_host(E: np.ndarray):
    """E [n, d] fp32 unit rows -> (idx int32 [n, P], cos float64 [n, P]): the lists of the rule (sdk_knn_rows)."""
    X = np.asarray(E, dtype=np.float32).astype(np.float64)
    n = X.shape[0]
    P = min(NMESC_P_MAX, n - 1)
    C = np.zeros((n, n))
    for t in range(X.shape[1]):
        C += X[:, t, None] * X[None, :, t]
    C = np.where(C == C, C, -np.inf)                                # a NaN ranks as -inf
    order = np.argsort(-C, axis=1, kind="stable")                   # ties to the lower j
    order = order[order != np.arange(n)[:, None]].reshape(n, n - 1)[:, :P]
    return order.astype(np.int32), np.take_along_axis(C, order, axis=1)


def knn_rows_fused_host(E_all: np.ndarray, maps: np.ndarray, weights):
    """E_all [n_all, d] fp32 unit rows, maps int [S, n], weights [S] float64 as the kernel receives them -> (idx int32 [n, P], f float64
    [n, P]): the lists of the fused affinity (sdk_knn_rows_fused), the same operations in the same order."""
    X = np.asarray(E_all, dtype=np.float32).astype(np.float64)
    maps = np.asarray(maps, dtype=np.int64)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if maps.ndim != 2 or maps.shape[0] != w.size or not 1 <= w.size <= _args.KNN_MAX_SCALES:
        raise ValueError(f"knn_rows_fused_host: maps must be [S, n] beside S weights, S in 1..{_args.KNN_MAX_SCALES}, got {list(maps.shape)} and {w.size}")
    out = np.argwhere((maps < 0) | (maps >= X.shape[0]))
    if out.size:
        raise ValueError(f"knn_rows_fused_host: base row {int(out[:, 1].min())} has a map entry outside [0, {X.shape[0]}) ({len(out)} such entries in all)")
    n = maps.shape[1]
    P = min(NMESC_P_MAX, n - 1)
    F = np.zeros((n, n))
    with np.errstate(invalid="ignore"):
        for s in range(w.size):
            A = X[maps[s]]
            C = np.zeros((n, n))
            for t in range(A.shape[1]):                             # knn_rows_host's chain, on the gathered rows
                C += A[:, t, None] * A[None, :, t]
            F = F + w[s] * C                                        # one rounded product, one rounded sum
    F = np.where(F == F, F, -np.inf)                                # a NaN ranks as -inf
    order = np.argsort(-F, axis=1, kind="stable")                   # ties to the lower j
    order = order[order != np.arange(n)[:, None]].reshape(n, n - 1)[:, :P]
    return order.astype(np.int32), np.take_along_axis(F, order, axis=1)


def knn_reverse_host(idx: np.ndarray):
    """idx [n, P] -> (rev_off int32 [n + 1], rev_src int32 [n P], rev_rank int32 [n P]): sdk_knn_reverse."""
    n, P = idx.shape
    tgt = idx.reshape(-1).astype(np.int64)
    src, rank = np.repeat(np.arange(n), P), np.tile(np.arange(P), n)
    order = np.lexsort((src, tgt))
    off = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=n))])
    return off.astype(np.int32), src[order].astype(np.int32), rank[order].astype(np.int32)


def knn_degree_host(rev_off: np.ndarray, rev_rank: np.ndarray, p: int):
    """-> (deg int32 [n], dinv float64 [n]): sdk_knn_degree."""
    n = rev_off.size - 1
    row = np.repeat(np.arange(n), np.diff(rev_off))
    deg = int(p) + np.bincount(row[rev_rank < p], minlength=n)
    return deg.astype(np.int32), 1.0 / np.sqrt(deg.astype(np.float64))


def knn_matvec_host(idx: np.ndarray, rev, dinv: np.ndarray, p: int, X: np.ndarray) -> np.ndarray:
    """Y = T_p X in the arithmetic sdk_knn_matvec states (include/sdk_hip.h): float64, row i's sum over its out-neighbours by rank, then over its
    reverse entries in stored order, every operation rounded once, the result rounded once to fp32."""
    rev_off, rev_src, rev_rank = rev
    n = idx.shape[0]
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    Z = dinv[:, None] * X64
    s = np.zeros_like(X64)
    for r in range(int(p)):
        s = s + Z[idx[:, r]]
    keep = rev_rank < p
    row = np.repeat(np.arange(n), np.diff(rev_off))[keep]
    src = rev_src[keep]
    first = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))])[:-1]
    pos = np.arange(row.size) - first[row]                          # the entry's place among its row's kept entries
    order = np.argsort(pos, kind="stable")
    cut = np.concatenate([[0], np.cumsum(np.bincount(pos, minlength=1))])
    for t in range(cut.size - 1):                                   # step t: every row's t-th entry (one entry per row at most)
        sl = order[cut[t]:cut[t + 1]]
        s[row[sl]] = s[row[sl]] + Z[src[sl]]
    return (0.5 * (X64 + dinv[:, None] * s)).astype(np.float32)


def knn_dense_host(idx: np.ndarray, p: int) -> np.ndarray:
    """The dense T_p [n, n] float64 of the lists' first p entries."""
    n = idx.shape[0]
    B = np.zeros((n, n))
    B[np.arange(n)[:, None], idx[:, :int(p)]] = 1.0
    A = B + B.T
    dinv = 1.0 / np.sqrt(A.sum(1))
    return 0.5 * (np.eye(n) + dinv[:, None] * A * dinv[None, :])


def _dense_top(idx: np.ndarray, p: int, m: int):
    """The m largest eigenvalues of T_p, descending, and their eigenvectors [n, m] (numpy.linalg.eigh, float64)."""
    lam, Q = np.linalg.eigh(knn_dense_host(idx, p))
    return lam[::-1][:m].copy(), Q[:, ::-1][:, :m].copy()


def _kmeans_host(R: np.ndarray, k: int, passes: int) -> np.ndarray:
    """_kmeans in numpy float64: maximin seeds from row 0 (ties to the lowest row), `passes` Lloyd passes (a centre without rows keeps its
    value), the labels of one more assignment (ties to the lowest centre)."""
    R = np.asarray(R, dtype=np.float64)
    centres = [R[0]]
    d2 = ((R - R[0]) ** 2).sum(1)
    for _ in range(1, k):
        j = int(np.argmax(d2))
        centres.append(R[j])
        d2 = np.minimum(d2, ((R - R[j]) ** 2).sum(1))
    C = np.stack(centres)

    def assign():
        return np.argmin(((R[:, None, :] - C[None, :, :]) ** 2).sum(2), axis=1)
    for _ in range(passes):
        lab = assign()
        for c in range(k):
            if (lab == c).any():
                C[c] = R[lab == c].mean(0)
    return assign()


def _pick_rows(who: str, R: int, rows):
    rows_h = np.arange(R, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    if rows_h.size and (rows_h.min() < 0 or rows_h.max() >= R or (np.diff(rows_h) <= 0).any()):
        raise ValueError(f"{who}: rows must ascend strictly inside [0, {R}), got {int(rows_h.min())} .. {int(rows_h.max())}")
    if rows_h.size > NMESC_MAX_ROWS:
        raise ValueError(f"{who}: {rows_h.size} rows (at most {NMESC_MAX_ROWS})")
    return rows_h


def _given_lists(who: str, rows, made):
    """The lists a `lists=` step made, (idx [n, P], values) -> (idx, n); such a step sees all of E, so `rows` has no meaning beside it."""
    if rows is not None:
        raise ValueError(f"{who}: rows and lists exclude each other (the lists step picks its own rows)")
    idx = made[0]
    n = int(idx.shape[0])
    if idx.ndim != 2 or n < 2 or n > NMESC_MAX_ROWS or int(idx.shape[1]) != min(NMESC_P_MAX, n - 1):
        raise ValueError(f"{who}: lists must return idx [n, min({NMESC_P_MAX}, n - 1)] with 2 <= n <= {NMESC_MAX_ROWS}, got {list(idx.shape)}")
    return idx, n


def nmesc_host(E, rows=None, speakers=None, neighbours=None, max_count: int = NMESC_MAX_COUNT, lists=None) -> NmescResult:
    """The whole rule in numpy float64, with the dense eigensolve at every n (so its eigenvalues are exact where nmesc_cluster's device path
    iterates): E [R, d] fp32 unit rows on the host, the other arguments nmesc_cluster's.  lists: as there, called as lists(E) ->
    (idx [n, P], values) on the host."""
    bounds = parse_speakers(speakers, "nmesc_host")
    E = np.asarray(E, dtype=np.float32)
    if lists is None:
        rows_h = _pick_rows("nmesc_host", E.shape[0], rows)
        X = E[rows_h]
        n = X.shape[0]
    else:
        idx, n = _given_lists("nmesc_host", rows, lists(E))
    m, _ = _nmesc_shape(max(n, 1), max_count)
    if n < 2:
        return NmescResult(np.zeros(n, np.int32), n, 0, (), np.zeros((0, m)), np.zeros(0), 0)
    if lists is None:
        bad = np.flatnonzero(~np.isfinite(X).all(1))
        if bad.size:
            raise ValueError(f"nmesc_host: row {int(bad[0])} has a non-finite value ({bad.size} such rows in all)")
    ps = nmesc_candidates(n, neighbours)
    if lists is None:
        idx, _ = knn_rows_host(X)
    tops = [_dense_top(idx, p, m) for p in ps]
    taus = np.stack([t[0] for t in tops])
    p_star, k_star, ratios, _ = nmesc_select(ps, taus, bounds, n)
    labels = np.zeros(n, np.int32)
    if k_star > 1:
        U = tops[ps.index(p_star)][1][:, :k_star]
        Rn = U / np.maximum(np.sqrt((U * U).sum(1, keepdims=True)), 1e-12)
        labels = canonical_labels(_kmeans_host(Rn, k_star, NMESC_KMEANS_PASSES)).astype(np.int32)
    return NmescResult(labels, k_star, p_star, ps, taus, ratios, 0)


def nmesc_cluster(provider, E, rows=None, speakers=None, neighbours=None, max_count: int = NMESC_MAX_COUNT, n_iter: int = NMESC_N_ITER,
                  seed: int = 0, lists=None) -> NmescResult:
    """Speaker clusters with neither a threshold nor a count: the rule stated above (E [R, d] fp32 unit rows on the provider's device; rows: the
    ascending row numbers that take part, host integers, None = all).  speakers: parse_speakers' bounds, part of the selection.  neighbours:
    the candidates in place of NMESC_NEIGHBOURS.  max_count: the most speakers looked for (1 .. THIN_MAX - 1).  The lists, their reverse, the
    degrees and every T_p V run in libsdk_hip.so (ops_cluster.knn_rows .. knn_matvec, csrc/nmesc.hip) beside the thin helpers of spectral_cluster.
    The host waits for the device result.host_reads times: the status of the lists, the eigenvalue table with the CholeskyQR flag (n <=
    NMESC_DENSE_ROWS: the lists instead), and the labels when k* > 1.  Fewer than two rows: one cluster or none, nothing launched.
    A single-process call: the rows are whole on this device and nothing is reduced across torch.distributed ranks.
    Ritz value i is converged to fp32 where (tau_{b+1} / tau_i)^(2 n_iter) is below 2^-24.  At the default n_iter = 30 that holds for the
    leading values of a clustered input, not for the bulk behind them (tau_{b+1} / tau_m of 0.8 .. 0.99 asks for 35 .. 900 steps): the
    table can then differ from nmesc_host's by a few 1e-3, and where two candidates' r(p) lie within that, p* can differ from
    nmesc_host's (k* and the labels rest on the leading gap).  n_iter, up to 1000, buys the agreement.
    lists: the step that makes the neighbour lists, None for the rule's own (knn_rows on the picked rows).  Given, it is called as
    lists(provider, E) and returns (idx int32 [n, P] on E's device, values), having made its one status read; n is then the number of
    lists, `rows` must be None, and everything behind the lists runs unchanged (nmesc_multiscale passes the fused affinity's)."""
    bounds = parse_speakers(speakers, "nmesc_cluster")
    if isinstance(n_iter, (bool, np.bool_)) or not isinstance(n_iter, (int, np.integer)) or not 0 <= n_iter <= 1000:
        raise ValueError(f"nmesc_cluster: n_iter={n_iter!r} (an int, 0 .. 1000)")
    if lists is None:
        rows_h = _pick_rows("nmesc_cluster", int(E.shape[0]), rows)
        n = int(rows_h.size)
    else:
        idx, n = _given_lists("nmesc_cluster", rows, lists(provider, E))             # read 1: the status
    m, b = _nmesc_shape(max(n, 1), max_count)
    if n < 2:
        return NmescResult(np.zeros(n, np.int32), n, 0, (), np.zeros((0, m)), np.zeros(0), 0)
    ps = nmesc_candidates(n, neighbours)
    dev = E.device
    if lists is None:
        Et = E if rows is None else E.index_select(0, torch.from_numpy(rows_h).to(dev)).contiguous()
        idx, _ = knn_rows(provider, Et)                                              # read 1: the status
    reads, comm, P = 1, _Comm(single=True), min(NMESC_P_MAX, n - 1)     # every rank that calls holds the whole problem: nothing is reduced
    retried = False
    if n <= NMESC_DENSE_ROWS:
        idx_h = idx.cpu().numpy()                                                   # read 2: the lists
        reads += 1
        tops = [_dense_top(idx_h, p, m) for p in ps]
        taus, n_iter = np.stack([t[0] for t in tops]), 0
    else:
        rev = knn_reverse(provider, idx, check_idx=False)                                # the lists are the kernel's own: no status read
        V0 = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, b)).astype(np.float32)).to(dev)
        spd_flag = torch.zeros((1,), dtype=torch.int32, device=dev)

        def ritz(p: int, shifted: bool):
            """-> (V [n, b] orthonormal after n_iter steps, Q [b, b], lam [b] descending) of T_p, on the device."""
            _, dinv = knn_degree(provider, rev[0], rev[2], P, p)
            V = _orth(provider, comm, V0, b, spd_flag, shifted)
            for _ in range(n_iter):
                V = _orth(provider, comm, knn_matvec(provider, idx, rev, dinv, p, V), b, spd_flag, shifted)
            Q, lam = provider.sym_eigh(provider.rows_gram(V, knn_matvec(provider, idx, rev, dinv, p, V)))
            return V, Q, lam

        def sweep(shifted: bool):
            table = torch.cat([ritz(p, shifted)[2][:m].double() for p in ps] + [spd_flag.double()]).cpu().numpy()      # ONE download
            return table[:-1].reshape(len(ps), m), bool(table[-1])
        taus, flagged = sweep(False)
        reads += 1
        if flagged and np.isfinite(taus).all() and hasattr(provider, "set_option"):
            spd_flag.zero_()                                                        # spectral_cluster's retry: shifted CholeskyQR
            retried = True
            taus, flagged = sweep(True)
            reads += 1
        if flagged or not np.isfinite(taus).all():
            raise np.linalg.LinAlgError(f"nmesc_cluster: the b = {b} block lost rank (Gram matrix not positive definite) on {n} rows")
    p_star, k_star, ratios, _ = nmesc_select(ps, taus, bounds, n)
    labels = np.zeros(n, np.int32)
    if k_star > 1:
        if n <= NMESC_DENSE_ROWS:
            U = torch.from_numpy(tops[ps.index(p_star)][1][:, :k_star].astype(np.float32)).to(dev).contiguous()
        else:
            V, Q, _ = ritz(p_star, retried)                                         # the same seed and block: the sweep's bits again
            U = provider.rows_apply(V, Q)[:, :k_star].contiguous()
        lab = _kmeans(provider, comm, provider.rows_unit(U), 0, n, k_star, NMESC_KMEANS_PASSES)
        labels = canonical_labels(lab.cpu().numpy()).astype(np.int32)               # the last read
        reads += 1
    return NmescResult(labels, k_star, p_star, ps, taus, ratios, int(n_iter), retried, reads)


def _multiscale_args(who: str, n_all: int, maps, weights):
    """maps on the host -> (maps int32 [S, n], the normalised weights float64 [S]) of the multi-scale rule."""
    maps_h = np.ascontiguousarray(maps)
    if maps_h.ndim != 2 or not np.issubdtype(maps_h.dtype, np.integer) or not 1 <= maps_h.shape[0] <= _args.KNN_MAX_SCALES:
        raise ValueError(f"{who}: maps must be integers [S, n] with S in 1..{_args.KNN_MAX_SCALES}, got {list(maps_h.shape)} {maps_h.dtype}")
    S, n = maps_h.shape
    if n > NMESC_MAX_ROWS:
        raise ValueError(f"{who}: {n} base rows (at most {NMESC_MAX_ROWS})")
    if n and (maps_h.min() < 0 or maps_h.max() >= n_all):
        raise ValueError(f"{who}: maps must lie in [0, {n_all}), got {int(maps_h.min())} .. {int(maps_h.max())}")
    w = np.asarray(_args.knn_weights(who, [1.0] * S if weights is None else weights, S), dtype=np.float64)
    return maps_h.astype(np.int32), w / w.sum()


def nmesc_multiscale_host(E_all, maps, weights=None, speakers=None, neighbours=None, max_count: int = NMESC_MAX_COUNT) -> NmescResult:
    """nmesc_multiscale in numpy float64 (nmesc_host on the fused affinity's lists): E_all [n_all, d] fp32 on the host."""
    E_all = np.asarray(E_all, dtype=np.float32)
    maps_h, w = _multiscale_args("nmesc_multiscale_host", E_all.shape[0], maps, weights)
    S, n = maps_h.shape
    if n < 2:
        res = nmesc_host(E_all[:0], None, speakers, neighbours, max_count)
        res.labels, res.n_speakers = np.zeros(n, np.int32), n
    else:
        bad = np.intersect1d(np.flatnonzero(~np.isfinite(E_all).all(1)), maps_h.reshape(-1))
        if bad.size:
            raise ValueError(f"nmesc_multiscale_host: row {int(bad[0])} of E_all, which a map names, has a non-finite value ({bad.size} such rows in all)")
        res = nmesc_host(E_all, None, speakers, neighbours, max_count, lists=lambda E: knn_rows_fused_host(E, maps_h, w))
    res.scales = S
    return res


def nmesc_multiscale(provider, E_all, maps, weights=None, speakers=None, neighbours=None, max_count: int = NMESC_MAX_COUNT,
                     n_iter: int = NMESC_N_ITER, seed: int = 0) -> NmescResult:
    """The eigengap clustering on the fused affinity of several window lengths: the multi-scale rule stated above NMESC_P_MAX.  E_all
    [n_all, d] fp32 unit rows of every scale stacked, on the provider's device; maps integers [S, n] (a host array, or an int32 device
    tensor, which is not read back): base window i's row of E_all at scale s; weights None (equal) or S numbers, normalised here.  The other arguments, the result and its
    host_reads are nmesc_cluster's (read 1 is the status of sdk_knn_rows_fused); result.scales = S.  Fewer than two base windows: one
    cluster or none, nothing launched."""
    on_device = isinstance(maps, torch.Tensor) and maps.is_cuda      # then it is not read back: the kernel's status answers for its range
    maps_h, w = _multiscale_args("nmesc_multiscale", int(E_all.shape[0]), np.zeros(tuple(maps.shape), np.int32) if on_device else maps, weights)
    S, n = maps_h.shape
    if n < 2:
        res = nmesc_cluster(provider, E_all[:0], None, speakers, neighbours, max_count, n_iter, seed)
        res.labels, res.n_speakers = np.zeros(n, np.int32), n
    else:
        maps_d = maps if on_device else torch.from_numpy(maps_h).to(E_all.device)
        res = nmesc_cluster(provider, E_all, None, speakers, neighbours, max_count, n_iter, seed,
                            lists=lambda eng, E: knn_rows_fused(eng, E, maps_d, w))
    res.scales = S
    return res
