"""The reference of tests/test_ahc_edges_gpu.py, checked on the CPU: on integer-lattice rows (ahc_ref.lattice) the float64 restatement
ahc_ref.centroid_linkage gives a valid tree whose steps are mostly exact ties, it agrees with the direct search of link_ref.linked_linkage,
and each of the tie rules it shares with csrc/ahc.hip decides the tree: a copy of the merge loop with one rule flipped gives another Z at
every size the GPU test compares, so a device kernel with that rule wrong cannot pass there."""
import numpy as np
import pytest

import ahc_ref
import link_ref

TIE_SIZES = (65, 129, 513)
# the row counts of test_ahc_edges_gpu.py's lattice cases up to 513 at which a rule can matter: with 2 rows there is one pair, and with 3
# rows the upkeep rule needs slots z < y < c and a dead x, four in all - those two sizes pin the edge, not the rules
RULE_SIZES = (63, 64, 65, 127, 128, 129, 511, 512, 513)


def _merge_loop(X, rescan_high=False, pair_high=False, no_upkeep=False, guess_y=False):
    """ahc_ref.centroid_linkage's loop (no gaps), with one tie rule flipped per switch: the rescan's ties to the highest j, the pair
    search's ties to the highest row, the `v == cur and y < c` upkeep dropped; guess_y: a row that pointed at x points at y (scipy's
    guess) where the rule leaves it without a neighbour.  All switches off: the restatement itself."""
    D = ahc_ref.distances(X)
    n = D.shape[0]
    Z = np.zeros((n - 1, 4))
    sz = np.ones(n, dtype=np.int64)
    ids = np.arange(n)
    nnd = np.full(n, np.inf)
    nn = np.full(n, -1)

    def rescan(r):
        js = np.flatnonzero(sz[r + 1:] > 0) + r + 1
        if js.size == 0:
            nnd[r], nn[r] = np.inf, -1
        else:
            row = D[r, js]
            k = js.size - 1 - int(np.argmin(row[::-1])) if rescan_high else int(np.argmin(row))
            nnd[r], nn[r] = row[k], js[k]

    for r in range(n - 1):
        rescan(r)
    for t in range(n - 1):
        while True:
            x = n - 1 - int(np.argmin(nnd[::-1])) if pair_high else int(np.argmin(nnd))
            y, dxy = int(nn[x]), float(nnd[x])
            if y >= 0 and D[x, y] == dxy:
                break
            rescan(x)
        nx, ny = int(sz[x]), int(sz[y])
        Z[t] = (min(ids[x], ids[y]), max(ids[x], ids[y]), dxy, nx + ny)
        z = np.flatnonzero(sz > 0)
        z = z[(z != x) & (z != y)]
        v = ahc_ref.lance_williams(D[x, z], D[y, z], dxy, nx, ny)
        D[y, z] = v
        D[z, y] = v
        lo = z < y
        zl, vl = z[lo], v[lo]
        c, cur = nn[zl], nnd[zl]
        lower = (vl < cur) if no_upkeep else (vl < cur) | ((vl == cur) & (y < c))
        nnd[zl[lower]] = vl[lower]
        nn[zl[lower]] = y
        nn[zl[~lower & (c == x)]] = y if guess_y else -1
        sz[x], sz[y], ids[y] = 0, nx + ny, n + t
        nnd[x], nn[x] = np.inf, -1
        rescan(y)
    return Z


@pytest.fixture(scope="module")
def ref():
    """{n: (X, Z, gaps)} of the restatement at the sizes the rules are judged at, computed once."""
    out = {}
    for n in RULE_SIZES:
        X = ahc_ref.tie_lattice(n)
        out[n] = (X,) + ahc_ref.centroid_linkage(X)
    return out


@pytest.mark.parametrize("n", TIE_SIZES)
def test_lattice_trees_are_valid_and_tie_rich(ref, n):
    X, Z, gaps = ref[n]
    ahc_ref.valid_tree(Z, n)
    ties, zeros, inv = int((gaps == 0).sum()), int((Z[:, 2] == 0).sum()), ahc_ref.inversions(Z)
    print(f"n={n} d={X.shape[1]}: {ties} of {n - 1} steps are exact ties, {zeros} zero heights, {inv} inversions")
    assert ties > n // 4
    assert zeros > 0
    assert inv > 0


@pytest.mark.parametrize("n", RULE_SIZES)
def test_want_gaps_off_gives_the_same_tree(ref, n):
    X, Z, _ = ref[n]
    Z0, g0 = ahc_ref.centroid_linkage(X, want_gaps=False)
    assert g0 is None and np.array_equal(Z0, Z)


@pytest.mark.parametrize("n", RULE_SIZES)
def test_each_tie_rule_decides_the_tree(ref, n):
    X, Z, _ = ref[n]
    assert np.array_equal(_merge_loop(X), Z), "the local copy is not the restatement"
    for flip in ("rescan_high", "pair_high", "no_upkeep"):
        Zf = _merge_loop(X, **{flip: True})
        first = np.flatnonzero((Zf != Z).any(axis=1))
        print(f"n={n}: {flip} changes {first.size} rows of Z, the first at step {first[0] if first.size else None}")
        assert first.size > 0, f"{flip} passes unnoticed at n={n}"


@pytest.mark.parametrize("n", [511, 512, 513])
def test_a_guessed_neighbour_is_not_the_rule(ref, n):
    """scipy's upkeep, which the kernel once followed: a row that pointed at the dead slot x is pointed at y with its bound kept.  When y
    happens to sit at that bound the guess is accepted although a lower slot may sit there too, and the tree then depends on the order of
    earlier merges.  That loop leaves the rule at these sizes (and at n = 129, d = 2), so the GPU comparison there tells the two apart."""
    X, Z, _ = ref[n]
    assert not np.array_equal(_merge_loop(X, guess_y=True), Z)
    X2 = ahc_ref.tie_lattice(129, 2)
    assert not np.array_equal(_merge_loop(X2, guess_y=True), ahc_ref.centroid_linkage(X2, want_gaps=False)[0])


@pytest.mark.parametrize("n", TIE_SIZES)
@pytest.mark.parametrize("grouped", [False, True])
def test_lazy_bounds_equal_the_direct_search(ref, n, grouped):
    """The lazy lower bounds of the restatement (and of the kernel) against link_ref's direct search of the least allowed pair, ties to the
    lowest slot and then the lowest neighbour: with every row free the two are the same rule, bit for bit.  With groups the direct search
    must keep them apart and end early."""
    X, Z, _ = ref[n]
    group = ahc_ref.tie_groups(n) if grouped else np.full(n, -1)
    Zl, m, gaps = link_ref.linked_linkage(X, group)
    if grouped:
        assert 0 < m < n - 1 and np.all(Zl[m:] == 0) and int((gaps == 0).sum()) > n // 4
        assert link_ref.no_group_twice(link_ref.labels_after(Zl, n, m), group)
    else:
        assert m == n - 1 and np.array_equal(Zl, Z)


@pytest.mark.parametrize("d", [1, 7, 33, 2048])
def test_lattice_distances_are_exact(d):
    """Squared lattice distances are integers below 2^53, so their float64 sum is exact in any order and D is the correctly rounded root of
    that integer: the one value any IEEE implementation gives.  (D ** 2 is NOT the integer again - sqrt(2) ** 2 = 2.0000000000000004 - so
    the comparison is with the root, and with the integer after rounding.)"""
    X = ahc_ref.lattice(129, d, 5)
    Xi = X.astype(np.int64)
    assert np.array_equal(Xi.astype(np.float32), X) and X.min() >= 0 and X.max() <= 3
    K = ((Xi[:, None, :] - Xi[None, :, :]) ** 2).sum(axis=2)
    D = ahc_ref.distances(X)
    assert np.array_equal(D, np.sqrt(K.astype(np.float64)))
    assert np.array_equal(np.rint(D ** 2).astype(np.int64), K)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0)
