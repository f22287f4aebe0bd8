"""Test-side checker of the centroid-linkage path (csrc/ahc.hip, cluster.agglomerative_cluster): a float64 numpy restatement of the
merge loop the GPU runs, recording at every step how far the runner-up pair was from the chosen one, and the threshold rule of
agglomerative_cluster restated on top of scipy's flat cut."""
from __future__ import annotations

import numpy as np


def distances(X: np.ndarray, block: int = 256) -> np.ndarray:
    """Square float64 Euclidean distances in difference form (never 2 - 2 x.y)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    D = np.empty((n, n))
    for a in range(0, n, block):
        diff = X[a:a + block, None, :] - X[None, :, :]
        D[a:a + block] = np.sqrt(np.einsum("ijk,ijk->ij", diff, diff))
    return D


def lance_williams(dxz, dyz, dxy, nx, ny):
    """scipy's _centroid, in its operation order, with the max(0, .) of the GPU path."""
    t = ((nx * dxz * dxz) + (ny * dyz * dyz)) - (float(nx * ny) * dxy * dxy) / (nx + ny)
    return np.sqrt(np.maximum(0.0, t / (nx + ny)))


def lattice(n: int, d: int, seed: int, hi: int = 4) -> np.ndarray:
    """n rows of d integer coordinates in [0, hi) as fp32: every squared difference and every partial sum of them is an exact float64 in any
    order, with or without fma, so the distances of two implementations agree bit for bit - and most merges are exact ties."""
    return np.random.default_rng(seed).integers(0, hi, (n, d)).astype(np.float32)


# tie_lattice's seed per row count: the least seed >= 0 whose lattice(n, 7, seed) holds a duplicate row (a zero height), has more than n // 4
# exactly tied steps and an inversion, and on which each of the three tie rules decides Z (tests/test_ahc_ref_cpu.py asserts all of it).
# Chosen from the restatement alone; any other row count takes seed n.
TIE_SEEDS = {63: 207, 64: 207, 65: 207, 127: 44, 128: 93, 129: 93, 511: 1, 512: 1, 513: 1}


def tie_lattice(n: int, d: int = 7) -> np.ndarray:
    return lattice(n, d, TIE_SEEDS.get(n, n))


def tie_groups(n: int) -> np.ndarray:
    """Groups for the linked linkage on tie_lattice: row i in group i % 5, every third row free (-1)."""
    g = (np.arange(n) % 5).astype(np.int32)
    g[::3] = -1
    return g


def centroid_linkage(X: np.ndarray, want_gaps: bool = True):
    """-> (Z [n-1, 4] in scipy's layout and numbering, gaps [n-1]): Muellner's generic algorithm as the GPU kernel runs it (nnd[i] a lower
    bound of row i's nearest live j > i, checked when it is the least; ties -> lowest row, lowest j).  Every step takes the live pair of
    least distance, ties to the lowest slot and then the lowest neighbour: link_ref.linked_linkage with every row free, which finds that
    pair by a direct search, gives the same Z bit for bit.
    gaps[t] = (runner-up pair distance - chosen distance) / chosen distance at step t (inf when no other pair is alive; 0 for a runner-up
    at the same distance, a zero distance included).  want_gaps=False skips the runner-up search (O(n^2) per step: unusable past ~1000 rows)
    and returns gaps = None; Z is the same."""
    D = distances(X)
    n = D.shape[0]
    Z = np.zeros((max(n - 1, 0), 4))
    gaps = np.full(max(n - 1, 0), np.inf) if want_gaps else None
    if n < 2:
        return Z, gaps
    sz = np.ones(n, dtype=np.int64)
    ids = np.arange(n)
    nnd = np.full(n, np.inf)
    nn = np.full(n, -1)

    def rescan(r):
        js = np.flatnonzero(sz[r + 1:] > 0) + r + 1
        if js.size == 0:
            nnd[r], nn[r] = np.inf, -1
        else:
            k = int(np.argmin(D[r, js]))
            nnd[r], nn[r] = D[r, js[k]], js[k]

    for r in range(n - 1):
        rescan(r)
    for t in range(n - 1):
        while True:                                    # nnd holds lower bounds: accept the least one only if it is exact
            x = int(np.argmin(nnd))
            y, dxy = int(nn[x]), float(nnd[x])
            if y >= 0 and D[x, y] == dxy:              # y < 0: the row's neighbour died and its bound was kept
                break
            rescan(x)
        if want_gaps:                                  # runner-up: the least live pair other than (x, y)
            live = np.flatnonzero(sz > 0)
            sub = D[np.ix_(live, live)]
            np.fill_diagonal(sub, np.inf)
            ix, iy = np.searchsorted(live, x), np.searchsorted(live, y)
            sub[ix, iy] = sub[iy, ix] = np.inf
            ru = sub.min()
            gaps[t] = (ru - dxy) / dxy if np.isfinite(ru) and dxy > 0 else (np.inf if not np.isfinite(ru) else 0.0)
        nx, ny = int(sz[x]), int(sz[y])
        Z[t] = (min(ids[x], ids[y]), max(ids[x], ids[y]), dxy, nx + ny)
        z = np.flatnonzero(sz > 0)
        z = z[(z != x) & (z != y)]
        v = lance_williams(D[x, z], D[y, z], dxy, nx, ny)
        D[y, z] = v
        D[z, y] = v
        lo = z < y
        zl, vl = z[lo], v[lo]
        c, cur = nn[zl], nnd[zl]
        lower = (vl < cur) | ((vl == cur) & (y < c))
        nnd[zl[lower]] = vl[lower]
        nn[zl[lower]] = y
        nn[zl[~lower & (c == x)]] = -1                 # bound kept, neighbour unknown: any live slot may sit at that bound
        sz[x], sz[y], ids[y] = 0, nx + ny, n + t
        nnd[x], nn[x] = np.inf, -1
        rescan(y)
    return Z, gaps


def inversions(Z: np.ndarray) -> int:
    return int((np.diff(Z[:, 2]) < 0).sum())


def canonical(lab) -> np.ndarray:
    lab = np.asarray(lab)
    _, first = np.unique(lab, return_index=True)
    order = lab[np.sort(first)]
    remap = {int(o): i for i, o in enumerate(order)}
    return np.array([remap[int(v)] for v in lab], dtype=np.int32)


def partition_after(Z: np.ndarray, n: int, merges: int) -> np.ndarray:
    """Canonical labels after the first `merges` rows of Z, by explicit member sets."""
    members = {i: {i} for i in range(n)}
    for t in range(merges):
        a, b = int(Z[t, 0]), int(Z[t, 1])
        members[n + t] = members.pop(a) | members.pop(b)
    lab = np.empty(n, dtype=np.int64)
    for k, m in members.items():
        lab[list(m)] = k
    return canonical(lab)


def threshold_rule(Z: np.ndarray, E: np.ndarray, threshold: float, min_cluster_size: int = 12, n_clusters=None) -> np.ndarray:
    """agglomerative_cluster's stated rule on a given linkage, with scipy's fcluster as the cut."""
    from scipy.cluster.hierarchy import fcluster
    N = E.shape[0]
    if N == 1:
        return np.zeros(1, np.int32)
    if n_clusters is not None:
        return partition_after(Z, N, N - min(max(n_clusters, 1), N))
    lab = canonical(fcluster(Z, threshold, "distance"))
    eff = min(min_cluster_size, max(1, round(0.1 * N)))
    K = lab.max() + 1
    sizes = np.array([(lab == k).sum() for k in range(K)])
    large = [k for k in range(K) if sizes[k] >= eff]
    if not large:
        return np.zeros(N, np.int32)
    E = np.asarray(E, dtype=np.float64)
    cent = {k: E[lab == k].mean(axis=0) for k in range(K)}
    out = lab.copy()
    for k in range(K):
        if sizes[k] >= eff:
            continue
        best, bd = None, None
        for L in large:
            d = 1.0 - cent[k] @ cent[L] / (np.linalg.norm(cent[k]) * np.linalg.norm(cent[L]))
            if bd is None or d < bd:
                best, bd = L, d
        out[lab == k] = best
    return canonical(out)


def valid_tree(Z: np.ndarray, n: int) -> None:
    """Every id 0 .. 2n-3 used exactly once, counts add up, heights finite and >= 0."""
    assert Z.shape == (n - 1, 4)
    used = Z[:, :2].astype(np.int64).ravel()
    assert np.array_equal(np.sort(used), np.arange(2 * n - 2)), "ids not used exactly once"
    size = np.ones(2 * n - 1, dtype=np.int64)
    for t in range(n - 1):
        a, b = int(Z[t, 0]), int(Z[t, 1])
        assert a < b < n + t, (t, a, b)
        size[n + t] = size[a] + size[b]
        assert Z[t, 3] == size[n + t], (t, Z[t, 3], size[n + t])
    assert np.isfinite(Z[:, 2]).all() and (Z[:, 2] >= 0).all()
