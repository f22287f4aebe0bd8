"""Test-side checker of the linked centroid linkage (csrc/ahc.hip's LINK kernels, sdk_linked_linkage, Engine.linked_linkage, cluster.link_rows,
diarize.link_speakers): a float64 numpy restatement of the rule that heads csrc/ahc.hip.  The device carries the constraint as +inf
distances; this restatement keeps every distance finite and decides what is forbidden from EXPLICIT MEMBER SETS (two clusters are forbidden
to each other when their members' non-negative groups intersect), so the two methods check each other.  Every step takes the least allowed
live pair directly (ties: lowest slot, then lowest neighbour) and records its relative gap to the runner-up among the allowed pairs."""
from __future__ import annotations

import numpy as np
import torch

import ahc_ref


def linked_linkage(X: np.ndarray, group, stop: float = np.inf):
    """-> (Z [n - 1, 4], merges, gaps [merges or merges + 1]): Z in scipy's layout and numbering, rows merges.. zero.  gaps[t] = (runner-up -
    chosen) / chosen among the allowed live pairs at step t (inf when no other allowed pair is alive); when the run ends on the stop rule, the
    step that was refused is recorded too (its pair was the minimum: a near-tie there could change nothing, but the gap is reported).
    `members[s]` is the set of rows of the cluster in slot s; forbiddance is read from the groups of those rows."""
    X = np.asarray(X)
    group = np.asarray(group, dtype=np.int64)
    n = X.shape[0]
    assert group.shape == (n,)
    Z = np.zeros((max(n - 1, 0), 4))
    gaps = []
    if n < 2:
        return Z, 0, np.asarray(gaps)
    D = ahc_ref.distances(X)
    sz = np.ones(n, dtype=np.int64)
    ids = np.arange(n)
    members = [{i} for i in range(n)]
    gsets = [({int(group[i])} if group[i] >= 0 else set()) for i in range(n)]

    def allowed(a, b):
        return gsets[a].isdisjoint(gsets[b])

    # W: the distance of every allowed live pair (x < y) at [x, y]; everything else +inf.  Derived from the member sets, rebuilt for slot y at a merge
    W = np.full((n, n), np.inf)
    for a in range(n):
        for b in range(a + 1, n):
            if allowed(a, b):
                W[a, b] = D[a, b]
    merges = 0
    for t in range(n - 1):
        k = int(np.argmin(W))                          # row-major first minimum: lowest slot, then lowest neighbour
        x, y = divmod(k, n)
        dxy = float(W[x, y])
        if not np.isfinite(dxy):
            break                                      # no allowed pair left
        W[x, y] = np.inf
        ru = float(W.min())
        W[x, y] = dxy
        gaps.append((ru - dxy) / dxy if np.isfinite(ru) and dxy > 0 else (np.inf if not np.isfinite(ru) else 0.0))
        if dxy > stop:
            break
        assert allowed(x, y) and sz[x] > 0 and sz[y] > 0 and x < y
        nx, ny = int(sz[x]), int(sz[y])
        Z[t] = (min(ids[x], ids[y]), max(ids[x], ids[y]), dxy, nx + ny)
        z = np.flatnonzero(sz > 0)
        z = z[(z != x) & (z != y)]
        v = ahc_ref.lance_williams(D[x, z], D[y, z], dxy, nx, ny)
        D[y, z] = v
        D[z, y] = v
        members[y] = members[x] | members[y]
        members[x] = set()
        gsets[y] = {int(group[i]) for i in members[y] if group[i] >= 0}
        gsets[x] = set()
        sz[x], sz[y], ids[y] = 0, nx + ny, n + t
        W[x, :] = np.inf
        W[:, x] = np.inf
        W[y, :] = np.inf
        W[:, y] = np.inf
        for q in z:
            if allowed(int(q), y):
                W[min(q, y), max(q, y)] = D[q, y]
        merges = t + 1
    return Z, merges, np.asarray(gaps)


def labels_after(Z: np.ndarray, n: int, merges: int) -> np.ndarray:
    return ahc_ref.partition_after(Z, n, merges)


def no_group_twice(labels, group) -> bool:
    """No cluster holds two rows of one non-negative group."""
    labels, group = np.asarray(labels), np.asarray(group)
    for c in np.unique(labels):
        g = group[labels == c]
        g = g[g >= 0]
        if len(np.unique(g)) != len(g):
            return False
    return True


class RefProvider:
    """cluster.link_rows' / diarize.link_speakers' provider on the CPU: the restatement behind Engine.linked_linkage's signature (one problem)."""
    def linked_linkage(self, E, group, offsets=None, stop=None):
        assert offsets is None
        E = E.numpy() if isinstance(E, torch.Tensor) else np.asarray(E)
        g = group.numpy() if isinstance(group, torch.Tensor) else np.asarray(group)
        Z, m, _ = linked_linkage(E, g, np.inf if stop is None else float(stop))
        return torch.from_numpy(Z), torch.tensor([m], dtype=torch.int32)


def planted(N: int, d: int, seed: int, per_rec: int = 3, n_id: int = 7, noise: float = 0.08):
    """N unit rows fp32 that look like per-recording centroids: recordings of per_rec rows (the last may be shorter), each row a distinct
    identity of a pool of n_id random unit vectors plus gaussian noise of size `noise`.  -> (X [N, d], group [N], identity [N])."""
    rng = np.random.default_rng(seed)
    pool = rng.standard_normal((n_id, d))
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)
    X, group, ident = [], [], []
    r = 0
    while len(X) < N:
        who = rng.permutation(n_id)[:per_rec]
        for w in who[:N - len(X)]:
            v = pool[w] + noise * rng.standard_normal(d) / np.sqrt(d)
            X.append(v / np.linalg.norm(v))
            group.append(r)
            ident.append(int(w))
        r += 1
    return np.asarray(X, dtype=np.float32), np.asarray(group, dtype=np.int32), np.asarray(ident)
