"""csrc/ahc.hip (distance, nearest-neighbour and merge kernels, and their LINK instantiations) bit for bit against the float64 restatements
tests/ahc_ref.py and tests/link_ref.py, on inputs where bit for bit is the only right answer, at the edges of the kernels' own constants.

The rows are ahc_ref.lattice: d small integers in [0, 4) as fp32.  Every squared difference and every partial sum is an exact float64 in any
order, with or without fma, so ahc_dist_kernel's D is ahc_ref.distances' bit for bit; from there the kernel computes scipy's _centroid
operation for operation under -ffp-contract=off, as ahc_ref.lance_williams does, and both sides state the same tie rules - and a large share
of the merge steps are exact ties (tests/test_ahc_ref_cpu.py counts them and shows each rule deciding the tree), so Z must be equal in all four
columns with np.array_equal: no margin, no rows left out.  The rows are NOT unit rows: the kernels use nothing that needs unit rows (the
distance is in difference form and Lance-Williams holds for any points), so none of these tests normalises.

Edges: TILE = 64 (63 / 64 / 65, 127 / 128 / 129), the nn sweep 64 U = 512 (511 / 512 / 513), the merge sweeps MERGE_THREADS U = 4096
(4096 / 4097; 4097 is also the first size whose per-row state passes 64 KiB of LDS and takes the opt-in), the state leaving LDS (8192 / 8193),
dim against KC = 32 (1, 2, 31, 32, 33, 63, 65, the limit 2048), ldE > dim, and a non-finite value in the last row of a partial tile and the
last column of a partial k-chunk."""
import time

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage

import ahc_ref
import link_ref
from conftest import sub

CL = sub("cluster")
pytestmark = pytest.mark.gpu

_ALONE = {}      # (n, d) -> the device's Z of ahc_ref.tie_lattice(n, d) alone, shared by the size tests and the batch test


def _dev(X, pad=0, fill=float("nan")):
    """X on the device; pad > 0: as the [:, :d] view of an [n, d + pad] buffer whose pad columns hold `fill`."""
    X = torch.from_numpy(np.ascontiguousarray(X))
    if not pad:
        return X.cuda()
    buf = torch.full((X.shape[0], X.shape[1] + pad), fill, dtype=torch.float32, device="cuda")
    buf[:, :X.shape[1]] = X.cuda()
    return buf[:, :X.shape[1]]


def _timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = f()
    out = tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()
    return out, time.perf_counter() - t


def _alone(engine, n, d=7):
    if (n, d) not in _ALONE:
        E = _dev(ahc_ref.tie_lattice(n, d))
        Z, s = _timed(lambda: engine.centroid_linkage(E))
        _ALONE[(n, d)] = (Z, s, int(E.stride(0)))
    return _ALONE[(n, d)]


def _against_restatement(engine, n, d, want_gaps):
    Z, s_dev, ld = _alone(engine, n, d)
    t = time.perf_counter()
    Zr, gaps = ahc_ref.centroid_linkage(ahc_ref.tie_lattice(n, d), want_gaps=want_gaps)
    s_ref = time.perf_counter() - t
    ties = f"{int((gaps == 0).sum())} of {n - 1}" if want_gaps else "not counted"
    print(f"n={n} d={d} ld={ld}: tie steps {ties}; device {s_dev:.3f} s, restatement {s_ref:.3f} s")
    assert Z.shape == (n - 1, 4)
    bad = np.flatnonzero((Z != Zr).any(axis=1))
    assert np.array_equal(Z, Zr), f"first differing step {bad[0]}: device {Z[bad[0]].tolist()}, restatement {Zr[bad[0]].tolist()}"


# ------------------------------------------------------------------------------------------------ rows: the tile and the nn sweep
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513])
def test_rows_at_tile_and_sweep_edges(engine, n):
    _against_restatement(engine, n, 7, True)


# ------------------------------------------------------------------------------------------------ the merge sweeps' stride and the LDS opt-in
@pytest.mark.parametrize("n", [4096, 4097])
def test_merge_sweep_stride_and_lds_optin(engine, n):
    _against_restatement(engine, n, 7, False)


# ------------------------------------------------------------------------------------------------ the per-row state in LDS / in the workspace
@pytest.mark.parametrize("n", [8192, 8193])
def test_state_in_lds_and_in_the_workspace(engine, n):
    """The full merge loop with the per-row state entirely in 128 KiB of LDS (8192) and in the workspace (8193)."""
    _against_restatement(engine, n, 7, False)


# ------------------------------------------------------------------------------------------------ columns
@pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 63, 65, 2048])
def test_columns_against_the_k_chunk(engine, d):
    """d = 1: at most four distinct rows, almost every step a tie at height zero.  2048 is the limit (include/sdk_hip.h: 1 <= dim <= 2048)."""
    _against_restatement(engine, 129, d, True)


@pytest.mark.parametrize("d", [2049, 4095])
def test_columns_past_the_limit_are_refused(engine, d):
    E = _dev(ahc_ref.lattice(3, d, 1))
    with pytest.raises(sub("_lib").SdkError, match=rf"dim={d} \(served: 1 \.\. 2048\)"):
        engine.centroid_linkage(E)
    with pytest.raises(sub("_lib").SdkError, match=rf"dim={d} \(served: 1 \.\. 2048\)"):
        engine.linked_linkage(E, torch.full((3,), -1, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------ leading dimension
@pytest.mark.parametrize("pad", [1, 5])
@pytest.mark.parametrize("d", [7, 33, 192])
def test_leading_dimension_past_dim(engine, d, pad):
    """E as a column view whose pad columns hold NaN: a kernel that reads one column past dim gives NaN distances (status 1: it raises)."""
    n = 129
    X = ahc_ref.tie_lattice(n, d)
    Z0 = _alone(engine, n, d)[0]
    E = _dev(X, pad)
    assert E.stride(0) == d + pad and E.stride(1) == 1 and not E.is_contiguous()
    Z, s = _timed(lambda: engine.centroid_linkage(E))
    print(f"n={n} d={d} ld={d + pad}: tie steps as contiguous; device {s:.3f} s")
    assert np.array_equal(Z, Z0)
    if pad == 1:                                                      # stride(1) != 1: the wrapper's .contiguous()
        Et = _dev(np.ascontiguousarray(X.T)).t()
        assert Et.shape == (n, d) and (d == 1 or Et.stride(1) != 1)
        assert np.array_equal(engine.centroid_linkage(Et).cpu().numpy(), Z0)


# ------------------------------------------------------------------------------------------------ batch across the LDS edge
def test_batch_on_both_sides_of_the_lds_state(engine):
    """lds_rows = 8192 for the launch: problems above it (state in the workspace) and below it (state in LDS) share one launch."""
    sizes = [8193, 65, 1, 4097, 2, 64]
    X = np.concatenate([ahc_ref.tie_lattice(n) for n in sizes])
    off = np.concatenate([[0], np.cumsum(sizes)])
    E = _dev(X)
    Z, s = _timed(lambda: engine.centroid_linkage(E, off))
    print(f"n={sizes} d=7 ld=7: device {s:.3f} s")
    assert Z.shape == (sum(sizes) - len(sizes), 4)
    for g, n in enumerate(sizes):
        Zg = Z[off[g] - g: off[g] - g + n - 1]
        if n > 1:
            assert np.array_equal(Zg, _alone(engine, n)[0]), g
        if 1 < n <= 513:
            assert np.array_equal(Zg, ahc_ref.centroid_linkage(ahc_ref.tie_lattice(n), want_gaps=False)[0]), g


# ------------------------------------------------------------------------------------------------ tie-free floats off the one shape
def test_tie_free_floats_equal_scipy(engine):
    n, d, ld = 129, 33, 40
    X = np.random.default_rng(129).standard_normal((n, d))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Zr, gaps = ahc_ref.centroid_linkage(X)
    Zs = linkage(X.astype(np.float64), "centroid")
    Z, s = _timed(lambda: engine.centroid_linkage(_dev(X, ld - d)))
    print(f"n={n} d={d} ld={ld}: tie steps {int((gaps == 0).sum())}, least gap {gaps.min():.3e}; device {s:.3f} s")
    assert gaps.min() > 1e4 * 1e-12, gaps.min()                      # every merge won by more than 1e4 x the height tolerance
    for ref in (Zs, Zr):
        assert np.array_equal(Z[:, [0, 1, 3]], ref[:, [0, 1, 3]]), "ids / counts differ"
        np.testing.assert_allclose(Z[:, 2], ref[:, 2], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ non-finite values at the edges
@pytest.mark.parametrize("where,bad", [((64, 32), float("nan")), ((0, 32), float("inf"))])
def test_non_finite_at_the_tile_and_chunk_edge(engine, where, bad):
    """n = 65: row 64 is the only row of the second tile; d = 33: column 32 is the only column of the second k-chunk."""
    n, d = 65, 33
    X = ahc_ref.tie_lattice(n, d)
    Xb = X.copy()
    Xb[where] = bad
    t = time.perf_counter()
    with pytest.raises(ValueError, match=r"centroid_linkage: problem 0 \(rows 0 \.\. 65\)") as ei:
        engine.centroid_linkage(_dev(Xb))
    assert ei.value.status.tolist() == [1]
    sizes = [n, 63, n]
    others = [ahc_ref.tie_lattice(63, d), X]
    off = np.concatenate([[0], np.cumsum(sizes)])
    with pytest.raises(ValueError, match=r"centroid_linkage: problem 0 \(rows 0 \.\. 65\)") as ei:
        engine.centroid_linkage(_dev(np.concatenate([Xb] + others)), off)
    print(f"n={sizes} d={d} ld={d}: {bad} at {where} of problem 0; {time.perf_counter() - t:.3f} s")
    assert ei.value.status.tolist() == [1, 0, 0]
    Z = ei.value.linkage.cpu().numpy()
    for g in (1, 2):
        assert np.array_equal(Z[off[g] - g: off[g] - g + sizes[g] - 1], _alone(engine, sizes[g], d)[0]), g


# ------------------------------------------------------------------------------------------------ the LINK kernels on ties
@pytest.mark.parametrize("n", [65, 129, 513])
def test_linked_kernels_on_ties(engine, n):
    X = ahc_ref.tie_lattice(n)
    group = ahc_ref.tie_groups(n)
    E, grp = _dev(X), torch.from_numpy(group).cuda()
    Zf, mf, gf = link_ref.linked_linkage(X, group)
    stop = float(np.median(Zf[:mf, 2]))
    for s, (Zr, mr, gaps) in ((None, (Zf, mf, gf)), (stop, link_ref.linked_linkage(X, group, stop))):
        (Z, m), sec = _timed(lambda: engine.linked_linkage(E, grp, None, s))
        print(f"n={n} d=7 ld=7 stop={s}: {mr} merges, tie steps {int((gaps == 0).sum())}; device {sec:.3f} s")
        assert 0 < mr < n - 1 and (s is None or mr < mf)
        assert m.tolist() == [mr]
        assert np.array_equal(Z, Zr) and np.all(Z[mr:] == 0)
        assert link_ref.no_group_twice(CL._flat_partition(Z, n, mr), group)
    free = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    (Z, m), sec = _timed(lambda: engine.linked_linkage(E, free, None, None))
    assert m.tolist() == [n - 1]
    assert np.array_equal(Z, ahc_ref.centroid_linkage(X, want_gaps=False)[0])
    assert np.array_equal(Z, _alone(engine, n)[0])
