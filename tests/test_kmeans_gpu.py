"""GPU checks of the k-means on unit rows (sdk_kmeans_rows, Engine.kmeans_rows, cluster.kmeans_cluster; csrc/kmeans.hip) against the numpy
float64 restatement of tests/kmeans_ref.py.  Each test prints its figures before it asserts.

The arithmetic bound (kmeans_bound): a row is assigned by comparing two cosines.  The kernel forms a cosine as d float64 fused multiply-adds
in column order of a unit row and a unit centre, so it is off the exact one by at most d 2^-53 (sum |e_j c_j| <= 1); the restatement rounds
every product and every sum, (d + 1) 2^-53 in round figures.  The two sides sum a centre's rows in the same stated order, so with equal
labels their sums are equal bit for bit and the centres differ by the norm alone: its sum of squares is taken in another order, (d + 2) 2^-53
relative, plus the roundings of the square root and of the division, (d + 4) 2^-53 on a cosine (the bound of test_centroids_against_float64).
Per cosine (3 d + 5) 2^-53, and two cosines are compared: (3 d + 5) 2^-52.  Seeds are rows: their products are exact in float64 and both
sides add them in column order, so the seeding is equal bit for bit and adds nothing."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as KR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
cluster = importlib.import_module(f"{PKG}.cluster")
LIB = importlib.import_module(f"{PKG}._lib")
pytestmark = pytest.mark.gpu


def kmeans_bound(d: int) -> float:
    return (3 * d + 5) * 2.0 ** -52


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def planted(seed: int, N: int, d: int, k: int, noise: float) -> np.ndarray:
    rng = np.random.default_rng(seed)
    cen = unit(rng.standard_normal((k, d))).astype(np.float64)
    return unit(cen[rng.integers(0, k, N)] + noise * rng.standard_normal((N, d)) / np.sqrt(d))


def same(a, b) -> bool:
    return (np.array_equal(a.labels, b.labels) and a.n_clusters == b.n_clusters and a.n_iter == b.n_iter and np.array_equal(a.counts, b.counts)
            and torch.equal(a.cent64, b.cent64) and torch.equal(a.cent, b.cent))


# ------------------------------------------------------------------------------------------------ one step, every shape
@pytest.mark.parametrize("N", [2, 255, 256, 257, 1000])
def test_one_step_equals_the_restatement(engine, N):
    """Seeded unit rows without structure, max_iters = 1: the labels are the first assignment from the maximin seeds.  Checked on the CPU for
    these seeds: the restatement's least margin over all shapes is 2.4e-7 (N = 1000, d = 64, k = 64), four orders over 10 x the bound, so no
    row is left out."""
    for d in (64, 192, 512):
        E = unit(np.random.default_rng(1000 * N + d).standard_normal((N, d)))
        Ed = dev(E)
        for k in sorted({kk for kk in (1, 2, 3, 64, N if N == 2 else 1) if kk <= N}):
            ref = KR.kmeans(E, k, max_iters=1)
            got = cluster.kmeans_cluster(engine, Ed, k, max_iters=1)
            bound = kmeans_bound(d)
            keep = ref["margins"][0] > 10 * bound
            left_out = int((~keep).sum())
            print(f"one step N={N} d={d} k={k}: bound {bound:.3e}; restatement's least margin {ref['least']:.3e} (10 x bound {10 * bound:.3e}); rows left out "
                  f"{left_out} of {N}; clusters {got.n_clusters} (restatement {ref['n_clusters']})")
            assert left_out <= 0.01 * N and got.n_iter == 1 == ref["n_iter"]
            if left_out == 0:
                assert np.array_equal(got.labels, ref["labels"]) and got.n_clusters == ref["n_clusters"] and np.array_equal(got.counts, ref["counts"])
            else:                                                         # compare through the raw centre numbers: canonical numbers may shift
                raw = engine.kmeans_rows(Ed, dev(np.arange(N, dtype=np.int32)), k, 1)[0].cpu().numpy()
                assert np.array_equal(raw[keep], ref["raw"][keep])
            assert int(got.labels.max()) + 1 == got.n_clusters <= k and got.counts.sum() == N and got.counts.min() >= 1


# widths at which the second column of a thread (j1 = tid + 256 of km_seed_pick, km_sums, km_finish) is live for one wave only (320) and for
# all waves but the last (448), at the one N that crosses the 256-row seed block and the 32-row assignment block; k = 64 fills the centre table
PARTIAL_ONE_STEP = [(257, d, k) for d in KR.PW.WIDTHS for k in (3, 64)]
PARTIAL_LOOP = (300, 320, 3, 13, 5.0)


def one_step_rows(N: int, d: int) -> np.ndarray:
    return unit(np.random.default_rng(1000 * N + d).standard_normal((N, d)))


@pytest.mark.parametrize("N,d,k", PARTIAL_ONE_STEP)
def test_one_step_where_the_second_column_is_partly_live(engine, N, d, k):
    """The one-step check at d = 320 and 448, with NO row left out.  Checked on the CPU (tests/test_speaker_bounds_cpu.py prints them): the
    restatement's least margins are 9.5e-5 (d = 320, k = 3), 3.6e-4 (320, 64), 1.2e-4 (448, 3) and 2.0e-4 (448, 64), seven orders over
    10 x the bound; without the columns 256.. the restatement gives other labels in all four cases."""
    E = one_step_rows(N, d)
    ref = KR.kmeans(E, k, max_iters=1)
    bound = kmeans_bound(d)
    print(f"one step N={N} d={d} k={k}: bound {bound:.3e}; restatement's least margin {ref['least']:.3e} (must exceed {10 * bound:.3e}, no row left out)")
    assert ref["least"] > 10 * bound and ref["n_iter"] == 1
    KR.second_column_weight(f"one step N={N} d={d} k={k}", E, k, (d + 4) * 2.0 ** -53, ref, max_iters=1)
    got = cluster.kmeans_cluster(engine, dev(E), k, max_iters=1)
    raw = engine.kmeans_rows(dev(E), dev(np.arange(N, dtype=np.int32)), k, 1)[0].cpu().numpy()
    e64 = float(np.abs(got.cent64.cpu().numpy() - ref["cent64"]).max()) if got.n_clusters == ref["n_clusters"] else np.inf
    print(f"  labels differing {int((got.labels != ref['labels']).sum())} of {N}; clusters {got.n_clusters} (restatement {ref['n_clusters']}); cent64 max|d| {e64:.3e} "
          f"(bound {(d + 4) * 2.0 ** -53:.3e}, ratio {e64 / ((d + 4) * 2.0 ** -53):.3f})")
    assert got.n_iter == 1 and np.array_equal(raw, ref["raw"])
    assert np.array_equal(got.labels, ref["labels"]) and got.n_clusters == ref["n_clusters"] and np.array_equal(got.counts, ref["counts"])
    assert int(got.labels.max()) + 1 == got.n_clusters <= k and got.counts.sum() == N and got.counts.min() >= 1
    assert e64 <= (d + 4) * 2.0 ** -53 and np.array_equal(got.cent.cpu().numpy(), got.cent64.cpu().numpy().astype(np.float32))


# ------------------------------------------------------------------------------------------------ the whole loop
@pytest.mark.parametrize("N,d,k,seed,noise", [(300, 192, 3, 11, 3.0), (1000, 256, 8, 12, 3.0), PARTIAL_LOOP])
def test_whole_loop_equals_the_restatement(engine, N, d, k, seed, noise):
    """Planted clusters: k seeded directions plus noise.  Checked on the CPU: with these seeds the restatement's least margin over ALL
    iterations is 2.6e-5 and 1.2e-5, seven orders over 10 x the bound, and the loop stops by itself after 6 and 5 of the 20 assignments.
    At d = 320 (the second column live for wave 0 only; tests/test_speaker_bounds_cpu.py prints its figures): least margin 1.2e-4 over
    8 assignments, and without the columns 256.. the restatement gives other labels."""
    E = planted(seed, N, d, k, noise)
    ref = KR.kmeans(E, k)
    bound = kmeans_bound(d)
    if d > KR.PW.FIRST:
        KR.second_column_weight(f"whole loop N={N} d={d} k={k}", E, k, (d + 4) * 2.0 ** -53, ref)
    got = cluster.kmeans_cluster(engine, dev(E), k)
    c64 = got.cent64.cpu().numpy()
    e64 = float(np.abs(c64 - ref["cent64"]).max())
    bound64 = (d + 4) * 2.0 ** -53
    print(f"whole loop N={N} d={d} k={k}: bound {bound:.3e}; restatement's least margin over {ref['n_iter']} iterations {ref['least']:.3e} (must exceed "
          f"{10 * bound:.3e}); n_iter gpu {got.n_iter}; counts {got.counts.tolist()}; cent64 max|d| {e64:.3e} (bound {bound64:.3e})")
    assert ref["least"] > 10 * bound and 2 <= ref["n_iter"] < cluster.KMEANS_MAX_ITERS
    assert np.array_equal(got.labels, ref["labels"]) and got.n_iter == ref["n_iter"] and np.array_equal(got.counts, ref["counts"])
    assert got.n_clusters == ref["n_clusters"] == k and e64 <= bound64
    assert np.array_equal(got.cent.cpu().numpy(), c64.astype(np.float32))
    twice = cluster.kmeans_cluster(engine, dev(E), k, max_iters=2 * cluster.KMEANS_MAX_ITERS)     # the stop on the device: more launches change nothing
    assert same(got, twice) and same(got, cluster.kmeans_cluster(engine, dev(E), k))


def test_more_than_one_segment_of_the_centre_sums(engine):
    """N = 2500 spans three 1024-row segments: the partials are added in segment order on both sides (8 assignments, least margin 3.4e-6
    in the restatement, checked on the CPU)."""
    E = planted(21, 2500, 64, 4, 3.0)
    ref = KR.kmeans(E, 4)
    got = cluster.kmeans_cluster(engine, dev(E), 4)
    print(f"segments N=2500 d=64 k=4: restatement's least margin {ref['least']:.3e} (must exceed {10 * kmeans_bound(64):.3e}); n_iter {got.n_iter}")
    assert ref["least"] > 10 * kmeans_bound(64) and ref["n_iter"] >= 2
    assert np.array_equal(got.labels, ref["labels"]) and got.n_iter == ref["n_iter"] and np.array_equal(got.counts, ref["counts"])


# ------------------------------------------------------------------------------------------------ ties, bit for bit
def test_tie_rules_bit_for_bit(engine):
    d = 64
    a, b, m = np.zeros(d, np.float32), np.zeros(d, np.float32), np.zeros(d, np.float32)
    a[0], b[1] = 1.0, 1.0
    m[0] = m[1] = 0.5                                                     # <m, a> = <m, b> = 0.5 exactly: the row straddles the two centres
    m[2] = np.float32(np.sqrt(0.5))
    E = np.stack([a, b, m, m])
    ref = KR.kmeans(E, 2, max_iters=1)
    assert ref["margins"][0][2] == 0.0 and ref["raw"].tolist() == [0, 1, 0, 0]
    for _ in range(2):
        raw = engine.kmeans_rows(dev(E), dev(np.arange(4, dtype=np.int32)), 2, 1)[0].cpu().numpy()
        assert raw.tolist() == [0, 1, 0, 0]                               # the tie goes to the lower centre
    mirrored = np.stack([b, a, m, m])
    assert engine.kmeans_rows(dev(mirrored), dev(np.arange(4, dtype=np.int32)), 2, 1)[0].cpu().numpy().tolist() == [0, 1, 0, 0]
    # two identical rows at k = 2: both seeds are row 0, every tie goes to centre 0, centre 1 is dropped
    row = unit(np.random.default_rng(3).standard_normal(d))
    two = cluster.kmeans_cluster(engine, dev(np.stack([row, row])), 2)
    assert two.labels.tolist() == [0, 0] and two.n_clusters == 1 and two.counts.tolist() == [2] and tuple(two.cent64.shape) == (1, d)
    assert KR.kmeans(np.stack([row, row]), 2)["n_clusters"] == 1 and two.n_iter == 2
    # k = N = 2 on two different rows: one each
    pair = cluster.kmeans_cluster(engine, dev(np.stack([a, b])), 2)
    assert pair.labels.tolist() == [0, 1] and pair.n_clusters == 2


# ------------------------------------------------------------------------------------------------ a subset of the rows
def test_rows_outside_the_subset_are_never_read(engine):
    N, d, k = 300, 192, 3
    E = planted(11, N, d, k, 3.0)
    rows = np.sort(np.random.default_rng(5).choice(2 * N, N, replace=False))
    big = np.full((2 * N, d), np.nan, np.float32)
    big[rows] = E
    full = cluster.kmeans_cluster(engine, dev(E), k)
    sub = cluster.kmeans_cluster(engine, dev(big), k, rows=rows)
    assert same(full, sub) and torch.isfinite(sub.cent64).all()


# ------------------------------------------------------------------------------------------------ a non-finite row, refusals
def test_non_finite_row_raises_after_the_read_and_the_engine_goes_on(engine):
    E = planted(11, 300, 192, 3, 3.0)
    for v in (np.nan, np.inf):
        bad = E.copy()
        bad[123, 77] = v
        with pytest.raises(ValueError, match="non-finite"):
            cluster.kmeans_cluster(engine, dev(bad), 3)
    ok = cluster.kmeans_cluster(engine, dev(E), 3)
    assert ok.n_clusters == 3 and np.array_equal(ok.labels, KR.kmeans(E, 3)["labels"])


def test_refusals_are_python_exceptions(engine):
    E = dev(planted(1, 10, 64, 2, 0.5))
    for k in (0, 65, 11, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match="k="):
            cluster.kmeans_cluster(engine, E, k)
    with pytest.raises(ValueError, match="d=100 not supported"):
        cluster.kmeans_cluster(engine, torch.zeros((10, 100), device="cuda"), 2)
    with pytest.raises(ValueError, match="fp32"):
        cluster.kmeans_cluster(engine, E.double(), 2)
    for rows in ([3, 1, 2], [1, 1, 2], [-1, 2], [2, 10]):
        with pytest.raises(ValueError, match="rows must ascend"):
            cluster.kmeans_cluster(engine, E, 2, rows=rows)
    with pytest.raises(ValueError, match="max_iters"):
        cluster.kmeans_cluster(engine, E, 2, max_iters=0)
    with pytest.raises(ValueError, match="k=3"):
        cluster.kmeans_cluster(engine, E, 3, rows=[0, 4])
    st = torch.cuda.current_stream().cuda_stream
    lib, z = engine.lib, torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rows = dev(np.arange(10, dtype=np.int32))
    assert lib.sdk_kmeans_rows_workspace_bytes(10, 100, 2) == 0 and lib.sdk_kmeans_rows_workspace_bytes(10, 64, 11) == 0
    assert 0 < lib.sdk_kmeans_rows_workspace_bytes(10, 64, 2) <= ws.numel()
    for n, d, k, it, msg in ((10, 100, 2, 5, "d=100 not supported"), (10, 64, 0, 5, "k=0"), (10, 64, 11, 5, "k=11"), (10, 64, 2, 0, "max_iters=0"),
                             (70000, 64, 2, 5, "n=70000")):
        with pytest.raises(LIB.SdkError, match=msg):
            LIB.check(lib.sdk_kmeans_rows(engine.ctx, E.data_ptr(), rows.data_ptr(), n, d, k, it, z.data_ptr(), z[1:].data_ptr(), z[2:].data_ptr(),
                                          ws.data_ptr(), ws.numel(), st), "sdk_kmeans_rows")
    with pytest.raises(LIB.SdkError, match="workspace of 16 bytes"):
        LIB.check(lib.sdk_kmeans_rows(engine.ctx, E.data_ptr(), rows.data_ptr(), 10, 64, 2, 5, z.data_ptr(), z[1:].data_ptr(), z[2:].data_ptr(),
                                      ws.data_ptr(), 16, st), "sdk_kmeans_rows")
    again = cluster.kmeans_cluster(engine, E, 2)                          # the device is fine after the refusals
    assert again.n_clusters == 2 and again.counts.sum() == 10
