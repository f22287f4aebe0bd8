"""Centroid-linkage agglomerative clustering (csrc/ahc.hip, sdk_centroid_linkage, Engine.centroid_linkage, cluster.agglomerative_cluster,
pipeline.run_shard(ahc_threshold=...), Backend.cluster_ranges).  The GPU's Z must be scipy's: ids and counts exactly, heights within
1e-12 relative; tests/ahc_ref.py restates the merge loop in float64 numpy and shows how far from a tie every step is."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import fcluster, linkage

import ahc_ref
from conftest import sub
from oracle.spectral import vmf_mixture

CL = sub("cluster")
PIPE = sub("pipeline")
T_PYANNOTE = 0.7045654963945799


def _unit_gauss(N, seed, d=192):
    X = np.random.default_rng(seed).standard_normal((N, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def _same_linkage(Z, Zs):
    assert Z.shape == Zs.shape, (Z.shape, Zs.shape)
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]]), "ids / counts differ from scipy"
    np.testing.assert_allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)


class _RefProvider:
    """agglomerative_cluster's provider on the CPU: the numpy restatement of the GPU merge loop."""
    def centroid_linkage(self, E):
        return torch.from_numpy(ahc_ref.centroid_linkage(E.numpy() if isinstance(E, torch.Tensor) else E)[0])


# ------------------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("N,k,noise", [(300, 6, 0.45), (800, 8, 0.5), (300, 0, 0.0)])
def test_ref_equals_scipy_with_margin(N, k, noise):
    X = vmf_mixture(N, 192, k, 11 + N, noise)[0] if k else _unit_gauss(N, 5)
    Z, gaps = ahc_ref.centroid_linkage(X)
    _same_linkage(Z, linkage(X.astype(np.float64), "centroid"))
    # every merge won by more than 1e4 x the height tolerance: an exact id comparison on the GPU is justified
    assert gaps.min() > 1e4 * 1e-12, gaps.min()
    assert ahc_ref.inversions(Z) > 0


def test_fcluster_distance_equals_scipy_with_inversions():
    for seed, noise in ((1, 0.45), (2, 0.55)):
        X = vmf_mixture(500, 192, 7, seed, noise)[0]
        Zs = linkage(X.astype(np.float64), "centroid")
        assert ahc_ref.inversions(Zs) > 50, "the data must exercise non-monotone heights"
        hs = np.sort(Zs[:, 2])
        for t in (T_PYANNOTE, 0.3, 0.5, 0.9, 1.2, float(hs[len(hs) // 2]), float(hs[-2]), 0.0, 10.0):
            want = ahc_ref.canonical(fcluster(Zs, t, "distance"))
            assert np.array_equal(CL.fcluster_distance(Zs, t), want), t


def test_rule_all_clusters_small_gives_one_label():
    lab = np.repeat(np.arange(20), 10)                     # N = 200: effective size min(12, 20) = 12, every cluster has 10
    E = _unit_gauss(200, 1).astype(np.float64)
    got, n_large = CL.fold_small_clusters(E, lab, 12)
    assert n_large == 0 and np.array_equal(got, np.zeros(200, np.int32))


def test_rule_tie_between_two_large_centroids_goes_to_the_lower_cluster():
    e1, e2 = np.eye(3)[0], np.eye(3)[1]
    mid = (e1 + e2) / np.sqrt(2.0)
    E = np.stack([e2] * 5 + [e1] * 5 + [mid])              # label 0 = the e2 cluster, label 1 = the e1 cluster, label 2 = one row between
    lab = np.array([0] * 5 + [1] * 5 + [2])
    got, n_large = CL.fold_small_clusters(E, lab, 3)       # N = 11: effective size min(3, 1) = 1 -> every cluster large
    assert n_large == 3 and np.array_equal(got, lab)
    got, n_large = CL.fold_small_clusters(E, lab, 12)      # min(12, round(1.1) = 1)... still 1
    assert n_large == 3
    E2 = np.concatenate([E[:10], E[:10], mid[None]])       # N = 21: effective size min(12, 2) = 2; the lone middle row is small
    lab2 = np.array([0] * 5 + [1] * 5 + [0] * 5 + [1] * 5 + [2])
    got, n_large = CL.fold_small_clusters(E2, lab2, 12)
    assert n_large == 2 and got[-1] == 0, got              # equal cosine to both: the large cluster first in label order


def test_rule_round_cap_half_to_even():
    E = _unit_gauss(35, 2).astype(np.float64)
    # N = 25: round(2.5) = 2 -> a 2-row cluster is large, a 1-row one is not
    lab = np.array([0] * 22 + [1, 1] + [2])
    got, n_large = CL.fold_small_clusters(E[:25], lab, 12)
    assert n_large == 2 and set(got[:24]) == {0, 1} and got[24] in (0, 1)
    # N = 35: round(3.5) = 4 -> a 3-row cluster is small
    lab = np.array([0] * 28 + [1] * 4 + [2] * 3)
    got, n_large = CL.fold_small_clusters(E, lab, 12)
    assert n_large == 2 and set(got) == {0, 1}
    # the cap never exceeds min_cluster_size
    lab = np.array([0] * 32 + [1] * 3)
    assert CL.fold_small_clusters(E, lab, 3)[1] == 2 and CL.fold_small_clusters(E, lab, 12)[1] == 1


def test_agglomerative_cluster_small_n_and_n_clusters():
    P = _RefProvider()
    one = CL.agglomerative_cluster(P, torch.from_numpy(_unit_gauss(1, 3)))
    assert np.array_equal(one.labels, [0]) and one.linkage.shape == (0, 4)
    two = torch.from_numpy(_unit_gauss(2, 4))
    d = float(np.linalg.norm(two[0].double() - two[1].double()))
    assert np.array_equal(CL.agglomerative_cluster(P, two, threshold=d + 0.01).labels, [0, 0])
    assert np.array_equal(CL.agglomerative_cluster(P, two, threshold=d - 0.01).labels, [0, 1])    # effective size 1: both large
    X = vmf_mixture(200, 192, 5, 9, 0.5)[0]
    Zs = linkage(X.astype(np.float64), "centroid")
    for k in (1, 2, 5, 17, 200):
        res = CL.agglomerative_cluster(P, torch.from_numpy(X), n_clusters=k, min_cluster_size=100)
        assert res.labels.max() + 1 == k
        assert np.array_equal(res.labels, ahc_ref.partition_after(Zs, 200, 200 - k)), k
    res = CL.agglomerative_cluster(P, torch.from_numpy(X), threshold=T_PYANNOTE)
    assert np.array_equal(res.labels, ahc_ref.threshold_rule(Zs, X, T_PYANNOTE))


def test_run_shard_refuses_both_clusterings():
    with pytest.raises(ValueError, match="n_clusters=3.*ahc_threshold=0.5"):
        PIPE.run_shard(None, None, None, n_clusters=3, ahc_threshold=0.5)


def test_cluster_ranges_refused_without_torch(monkeypatch):
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    be = sub("backend").Backend()
    with pytest.raises(ValueError, match="cluster_ranges"):
        be.cluster_ranges(np.zeros(32000, np.int16), [(0.0, 2.0)])


# ------------------------------------------------------------------------------------------------------------------------------- GPU
def _gpu_Z(engine, X, offsets=None):
    E = engine.l2norm(torch.from_numpy(np.ascontiguousarray(X)).cuda())[0]
    Z = engine.centroid_linkage(E, offsets)
    return E, Z.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 3, 17, 300, 2000, 5000])
@pytest.mark.parametrize("kind", ["mixture", "gaussian"])
def test_gpu_linkage_equals_scipy(engine, N, kind):
    X = vmf_mixture(N, 192, max(2, min(12, N // 40)), 100 + N, 0.5)[0] if kind == "mixture" else _unit_gauss(N, 200 + N)
    E, Z = _gpu_Z(engine, X)
    _same_linkage(Z, linkage(E.cpu().numpy().astype(np.float64), "centroid"))


@pytest.mark.gpu
def test_gpu_batch_equals_alone_and_scipy(engine):
    sizes = [300, 1, 17, 2, 1000, 3, 64]
    X = np.concatenate([vmf_mixture(n, 192, 4, 7 + i, 0.5)[0] for i, n in enumerate(sizes)])
    off = np.concatenate([[0], np.cumsum(sizes)])
    E, Z = _gpu_Z(engine, X, off)
    assert Z.shape == (sum(sizes) - len(sizes), 4)
    Eh = E.cpu().numpy().astype(np.float64)
    for g, n in enumerate(sizes):
        Zg = Z[off[g] - g: off[g] - g + n - 1]
        alone = engine.centroid_linkage(E[off[g]:off[g + 1]].contiguous()).cpu().numpy()
        assert np.array_equal(Zg, alone), g                                   # bit for bit
        if n > 1:
            _same_linkage(Zg, linkage(Eh[off[g]:off[g + 1]], "centroid"))


@pytest.mark.gpu
def test_gpu_duplicate_rows_same_cut_as_scipy(engine):
    base = vmf_mixture(120, 192, 4, 21, 0.45)[0]
    rep = np.random.default_rng(3).integers(1, 4, size=120)
    X = np.repeat(base, rep, axis=0)
    X = X[np.random.default_rng(4).permutation(X.shape[0])]
    E, Z = _gpu_Z(engine, X)
    ahc_ref.valid_tree(Z, X.shape[0])
    Zs = linkage(E.cpu().numpy().astype(np.float64), "centroid")
    for t in (0.0, 1e-9, 0.3, T_PYANNOTE, 1.0, 5.0):
        assert np.array_equal(CL.fcluster_distance(Z, t), ahc_ref.canonical(fcluster(Zs, t, "distance"))), t


@pytest.mark.gpu
def test_gpu_agglomerative_cluster_follows_the_rule(engine):
    for N, k, noise, t, m in ((400, 6, 0.5, T_PYANNOTE, 12), (1500, 9, 0.55, T_PYANNOTE, 12), (300, 5, 0.5, 0.6, 40)):
        X = vmf_mixture(N, 192, k, N + k, noise)[0]
        E = engine.l2norm(torch.from_numpy(X).cuda())[0]
        res = CL.agglomerative_cluster(engine, E, t, m)
        Eh = E.cpu().numpy().astype(np.float64)
        Zs = linkage(Eh, "centroid")
        _same_linkage(res.linkage, Zs)
        assert np.array_equal(res.labels, ahc_ref.threshold_rule(Zs, Eh, t, m)), (N, k)


def _tight(N, k, seed):
    X, lab = vmf_mixture(N, 192, k, seed, 0.02)
    return X, lab


@pytest.mark.gpu
def test_gpu_largest_problem(engine):
    N = 65536
    X, truth = _tight(N, 6, 31)
    E, Z = _gpu_Z(engine, X)
    ahc_ref.valid_tree(Z, N)
    assert np.array_equal(CL.fcluster_distance(Z, 0.5), truth)               # ARI 1: canonical labels equal


@pytest.mark.gpu
def test_gpu_batch_past_2_31_distances(engine):
    sizes = [46400, 46401]
    assert sum(n * n for n in sizes) > 2 ** 31
    parts = [_tight(n, 5 + g, 40 + g) for g, n in enumerate(sizes)]
    X = np.concatenate([p[0] for p in parts])
    off = np.concatenate([[0], np.cumsum(sizes)])
    E, Z = _gpu_Z(engine, X, off)
    for g, n in enumerate(sizes):
        Zg = Z[off[g] - g: off[g] - g + n - 1]
        ahc_ref.valid_tree(Zg, n)
        assert np.array_equal(CL.fcluster_distance(Zg, 0.5), parts[g][1]), g


@pytest.mark.gpu
def test_gpu_nan_row_names_its_problem(engine):
    sizes = [200, 150, 90]
    X = np.concatenate([vmf_mixture(n, 192, 3, 60 + i, 0.5)[0] for i, n in enumerate(sizes)])
    off = np.concatenate([[0], np.cumsum(sizes)])
    E = engine.l2norm(torch.from_numpy(X).cuda())[0]
    E[200 + 37, 5] = float("nan")
    with pytest.raises(ValueError, match=r"problem 1 \(rows 200 \.\. 350\)") as ei:
        engine.centroid_linkage(E, off)
    Z = ei.value.linkage.cpu().numpy()
    Eh = E.cpu().numpy().astype(np.float64)
    for g in (0, 2):
        _same_linkage(Z[off[g] - g: off[g] - g + sizes[g] - 1], linkage(Eh[off[g]:off[g + 1]], "centroid"))
    E[200 + 37, 5] = float("inf")
    with pytest.raises(ValueError, match="problem 1"):
        engine.centroid_linkage(E, off)


@pytest.mark.gpu
def test_gpu_refusals_name_the_value_and_launch_nothing(engine):
    lib = engine.lib
    SENT = -7.25
    E = engine.l2norm(torch.from_numpy(vmf_mixture(64, 192, 3, 1, 0.5)[0]).cuda())[0]
    Z = torch.full((80, 4), SENT, dtype=torch.float64, device="cuda")
    st = torch.full((4,), 99, dtype=torch.int32, device="cuda")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")

    def offs(*v):
        a = np.array(v, dtype=np.int32)
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    def refused(pats, E_=None, ld=192, dim=192, off=(0, 64), G=None, Z_=None, st_=None, ws_=None, wsb=None):
        a, p = offs(*off)
        G = len(off) - 1 if G is None else G
        rc = lib.sdk_centroid_linkage(engine.ctx, E.data_ptr() if E_ is None else E_, ld, dim, p, G, Z.data_ptr() if Z_ is None else Z_,
                                      st.data_ptr() if st_ is None else st_, ws.data_ptr() if ws_ is None else ws_, ws.numel() if wsb is None else wsb, None)
        msg = lib.sdk_last_error().decode()
        assert rc != 0 and "sdk_centroid_linkage" in msg, (rc, msg)
        for q in pats:
            assert q in msg, (q, msg)

    refused(["null argument"], Z_=0)
    refused(["null argument"], ws_=0)
    refused(["misaligned", f"E={E.data_ptr() + 2:#x}"], E_=E.data_ptr() + 2)
    refused(["misaligned", f"Z={Z.data_ptr() + 4:#x}"], Z_=Z.data_ptr() + 4)
    refused(["misaligned"], ws_=ws.data_ptr() + 16)
    refused(["G=0"], G=0)
    refused(["offsets not increasing at problem 1", "offsets[2]=30"], off=(0, 40, 30, 64))
    refused(["offsets not increasing at problem 0"], off=(0, 0, 64))
    refused(["problem 0 has n=65537 rows", "65536"], off=(0, 65537))
    refused(["offsets[0]=8"], off=(8, 64))
    refused(["dim=0"], dim=0)
    refused(["dim=4096"], dim=4096, ld=4096)
    refused(["ldE=100 < dim=192"], ld=100)
    need = lib.sdk_centroid_linkage_workspace_bytes(offs(0, 64)[1], 1, 192)
    assert need > 64 * 64 * 8
    refused(["workspace of", str(need)], wsb=need - 1)
    assert lib.sdk_centroid_linkage_workspace_bytes(offs(0, 65537)[1], 1, 192) == 0
    torch.cuda.synchronize()
    assert bool((Z.cpu() == SENT).all()) and bool((st.cpu() == 99).all()), "a refused call launched"
    # the context is intact
    Zok = engine.centroid_linkage(E).cpu().numpy()
    _same_linkage(Zok, linkage(E.cpu().numpy().astype(np.float64), "centroid"))


@pytest.mark.gpu
def test_gpu_run_shard_ahc_equals_agglomerative_cluster(engine):
    rng = np.random.default_rng(8)
    S = 32000
    t = np.arange(S) / 16000.0
    pcm = np.concatenate([np.clip(np.round((rng.normal(0, 0.05, (8, S)) + 0.3 * np.sin(2 * np.pi * f * t)) * 32768), -32768, 32767)
                          for f in (180.0, 330.0, 520.0)]).astype(np.int16)
    profiles = torch.from_numpy(rng.standard_normal((4, 192)).astype(np.float32)).cuda()
    out = PIPE.run_shard(engine, torch.from_numpy(pcm).cuda(), profiles, ahc_threshold=0.5, ahc_min_cluster_size=3)
    res = CL.agglomerative_cluster(engine, out.embeddings, 0.5, 3)
    assert np.array_equal(out.cluster_labels, res.labels)
    assert np.array_equal(out.linkage, res.linkage) and out.linkage.shape == (pcm.shape[0] - 1, 4)


@pytest.mark.gpu
def test_gpu_backend_cluster_ranges(tmp_path, monkeypatch):
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    be = sub("backend").Backend()
    rng = np.random.default_rng(12)
    sr = 16000
    t = np.arange(sr * 3) / sr
    parts = [np.round((0.25 * np.sin(2 * np.pi * f * t) + rng.normal(0, 0.03, t.size)) * 32768) for f in (200.0, 600.0, 200.0, 600.0)]
    samples = np.clip(np.concatenate(parts), -32768, 32767).astype(np.int16)
    ranges = [(0.0, 3.0), (3.0, 6.0), (6.0, 9.0), (9.0, 12.0), (12.0, 12.2)]
    labels, wins, rl = be.cluster_ranges(samples, ranges, threshold=0.3, min_cluster_size=2)
    E, _, _, wins2, _ = be.embed_ranges(samples, ranges)
    want = CL.agglomerative_cluster(be.engine(), E, 0.3, 2).labels
    assert wins == wins2 and np.array_equal(labels, want)
    assert rl.shape == (5,) and rl[4] == -1
    for ri in range(4):
        lab = [int(l) for (r, _, _), l in zip(wins, labels) if r == ri]
        assert rl[ri] == int(np.argmax(np.bincount(lab)))
