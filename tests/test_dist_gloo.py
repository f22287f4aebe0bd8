"""N > 1 path on CPU: world_size-2 gloo processes exercise the sharding + all-gather plumbing that
bench.py / the clustering stage use over RCCL on the GPUs."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, n_total, out_dir):
    import importlib
    import sys
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    D = importlib.import_module(f"{PKG}.dist")
    full = torch.from_numpy(np.random.default_rng(0).standard_normal((n_total, 192)).astype(np.float32))
    lo, hi = D.shard_range(n_total)
    gathered = D.all_gather_rows(full[lo:hi].clone(), n_total)
    ok = torch.equal(gathered, full)
    s = D.all_reduce_sum(torch.tensor([float(hi - lo)]))
    ok = ok and int(s.item()) == n_total
    # ragged + empty shards
    lo1, hi1 = D.shard_range(1)                       # rank 0 owns the only row, rank 1 an empty shard
    g2 = D.all_gather_rows(full[lo1:hi1].clone(), 1)
    ok = ok and torch.equal(g2, full[:1])
    # the pairwise form of the exchange ($SDK_ALLGATHER=direct: world - 1 send / receive pairs in one batch) gathers the same bytes
    os.environ["SDK_ALLGATHER"] = "direct"
    ok = ok and D.allgather_mode() == "direct" and torch.equal(D.all_gather_rows(full[lo:hi].clone(), n_total), full)
    ok = ok and torch.equal(D.all_gather_rows(full[lo1:hi1].clone(), 1), full[:1])
    os.environ["SDK_ALLGATHER"] = "auto"
    w = max(h - l for l, h in D.shard_bounds(n_total, world))
    pad = torch.zeros(w, 192); pad[:hi - lo] = full[lo:hi]
    a, b = torch.empty(world * w, 192), torch.empty(world * w, 192)
    D._gather_into(a, pad, mode="auto"); D._gather_into(b, pad, mode="direct")
    ok = ok and torch.equal(a, b)
    open(os.path.join(out_dir, f"rank{rank}.ok" if ok else f"rank{rank}.bad"), "w").close()
    dist.destroy_process_group()


def test_shard_bounds_cover_rows_exactly():
    import importlib
    D = importlib.import_module(f"{PKG}.dist")
    for n in (0, 1, 7, 8, 1000, 1_000_003):
        for w in (1, 2, 3, 8):
            b = D.shard_bounds(n, w)
            assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(w - 1))
            sizes = [h - l for l, h in b]
            assert max(sizes) - min(sizes) <= 1
    assert D.shard_bounds(1_000_000, 8)[3] == (375_000, 500_000)     # config #4: 125k segments per GPU


@pytest.mark.parametrize("world", [2, 3])
def test_all_gather_rows_world2_gloo(tmp_path, world):
    for n_total in (11, 64):
        d = tmp_path / f"n{n_total}"
        d.mkdir()
        mp.spawn(_worker, args=(world, _free_port(), n_total, str(d)), nprocs=world, join=True)
        assert sorted(os.listdir(d)) == [f"rank{r}.ok" for r in range(world)]


def _cluster_worker(rank, world, port, out_dir):
    import importlib
    import sys
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cpu_provider import CpuProvider
    from oracle import spectral as ospec
    D = importlib.import_module(f"{PKG}.dist")
    CL = importlib.import_module(f"{PKG}.cluster")
    N, k = 601, 4                                         # odd N: ragged shards
    E, truth = ospec.vmf_mixture(N, 192, k, seed=11, noise=0.5)
    Eb = torch.from_numpy(E).to(torch.bfloat16)
    lo, hi = D.shard_range(N)
    res = CL.spectral_cluster(CpuProvider(), torch.from_numpy(E[lo:hi]), Eb[lo:hi].clone(), N, k, n_iter=20, n_kmeans=15, seed=0)
    olab, olam = ospec.spectral_cluster(Eb.float().numpy(), k, n_iter=20, n_kmeans=15, seed=0)
    ok = np.array_equal(res.labels, olab) and np.abs(res.eigenvalues - olam).max() < 1e-5 and ospec.adjusted_rand_index(res.labels, truth) == 1.0
    open(os.path.join(out_dir, f"rank{rank}.ok" if ok else f"rank{rank}.bad"), "w").close()
    dist.destroy_process_group()


def test_spectral_cluster_world2_gloo(tmp_path):
    """Row-sharded spectral clustering (embedding all-gather, per-iteration V all-gather, Gram and centroid
    all-reduces) on two CPU ranks: every rank must reproduce the single-process oracle's integer labels."""
    mp.spawn(_cluster_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["rank0.ok", "rank1.ok"]


def test_spectral_cluster_single_process_cpu_provider():
    import importlib
    import sys
    sys.path.insert(0, str(ROOT / "tests"))
    from cpu_provider import CpuProvider
    from oracle import spectral as ospec
    CL = importlib.import_module(f"{PKG}.cluster")
    E, truth = ospec.vmf_mixture(500, 192, 5, seed=3, noise=0.5)
    Eb = torch.from_numpy(E).to(torch.bfloat16)
    res = CL.spectral_cluster(CpuProvider(), torch.from_numpy(E), Eb, 500, 5, n_iter=20, n_kmeans=15)
    olab, olam = ospec.spectral_cluster(Eb.float().numpy(), 5, n_iter=20, n_kmeans=15)
    assert np.array_equal(res.labels, olab) and np.abs(res.eigenvalues - olam).max() < 1e-5
    assert ospec.adjusted_rand_index(res.labels, truth) == 1.0


def test_spectral_cluster_raises_on_a_flagged_gram_matrix():
    """cluster.py's side of the sync-free CholeskyQR: a provider that only SETS the sticky device flag (what ops.Engine
    does) must still end in LinAlgError at the Ritz step, and a provider that raises by itself (the CPU stand-in) propagates."""
    import importlib
    import sys
    sys.path.insert(0, str(ROOT / "tests"))
    from cpu_provider import CpuProvider
    CL = importlib.import_module(f"{PKG}.cluster")

    class Flagging(CpuProvider):
        def chol_inverse(self, G, flag=None):
            try:
                return super().chol_inverse(G)
            except np.linalg.LinAlgError:
                flag.fill_(1)
                return torch.eye(G.shape[0])

    rng = np.random.default_rng(0)
    base = rng.standard_normal((3, 192)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    E = np.repeat(base, 50, axis=0)
    Eb = torch.from_numpy(E).to(torch.bfloat16)
    for prov in (Flagging(), CpuProvider()):
        with pytest.raises(np.linalg.LinAlgError):
            CL.spectral_cluster(prov, torch.from_numpy(E), Eb, 150, 6, n_iter=4, n_kmeans=3)
    res = CL.spectral_cluster(Flagging(), torch.from_numpy(E), Eb, 150, 3, n_iter=6, n_kmeans=3)
    assert np.array_equal(res.labels, np.repeat(np.arange(3), 50))


def test_bench_gpus_n_spawns_its_own_ranks_before_any_gpu_call(monkeypatch):
    """VERDICT r3 next #2b: the driver runs `python bench.py --gpus N ...` directly.  Without a rank environment bench.py becomes the launcher:
    N children through torch.distributed.run on 127.0.0.1, the original flags passed on, the children's exit code returned, and no GPU call
    in the parent (a process that has initialised the GPU must never be replaced or re-exec'ed)."""
    import subprocess
    import sys as _sys
    import torch
    _sys.path.insert(0, str(ROOT))
    import bench
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3", "--warmup", "1"])
    assert bench.main() == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [_sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "8", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert not torch.cuda.is_initialized()
    # with a rank environment that disagrees with the flag it is still a usage error, not a second launcher
    monkeypatch.setenv("WORLD_SIZE", "2")
    seen.clear()
    assert bench.main() == 2 and not seen


def test_bench_rccl_path_refuses_more_ranks_than_devices(monkeypatch, capsys):
    """`--gpus N` with fewer than N visible devices must end in a readable message before set_device (here: 0 devices,
    world 2, the rank environment of torch.distributed.run), not in a HIP error or an RCCL hang; the gloo rehearsal path is not refused."""
    import sys as _sys
    import torch
    _sys.path.insert(0, str(ROOT))
    import bench
    for k, v in (("WORLD_SIZE", "2"), ("RANK", "0"), ("LOCAL_RANK", "0"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29999")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("SDK_BENCH_BACKEND", raising=False)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    called = []
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: called.append(d))
    assert bench.main() == 2 and not called
    err = capsys.readouterr().err
    assert "needs 2 visible GPUs" in err and "shows 1" in err and "SDK_BENCH_BACKEND=gloo" in err


def test_bench_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: every array as DIR/<name>.npy, integers as float64 and floats as float32, values unchanged; past the
    byte budget each array is cut to a seeded sample of its rows (the same rows on every run and for arrays of equal length, their numbers
    beside them) and the files stay inside the budget."""
    import sys as _sys
    import torch
    _sys.path.insert(0, str(ROOT))
    import bench
    E = torch.randn(500, 192, generator=torch.Generator().manual_seed(0))
    ids = torch.arange(500, dtype=torch.int32).reshape(-1, 1)
    sc = torch.rand(500, 1, generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path / "all"), {"embeddings": E, "ids": ids, "scores": sc})
    got = {n: np.load(tmp_path / "all" / f"{n}.npy") for n in ("embeddings", "ids", "scores")}
    assert sorted(p.name for p in (tmp_path / "all").iterdir()) == ["embeddings.npy", "ids.npy", "scores.npy"]
    assert got["embeddings"].dtype == np.float32 and got["scores"].dtype == np.float32 and got["ids"].dtype == np.float64
    assert np.array_equal(got["embeddings"], E.numpy()) and np.array_equal(got["ids"], ids.numpy()) and np.array_equal(got["scores"], sc.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100_000)
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), {"embeddings": E, "ids": ids, "scores": sc})
        assert sum(p.stat().st_size for p in (tmp_path / run).iterdir()) <= 100_000
    rows = np.load(tmp_path / "s1" / "embeddings_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 500 and np.array_equal(rows, np.load(tmp_path / "s2" / "embeddings_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "embeddings.npy"), E.numpy()[rows])
    # arrays of the same length keep the same rows: the sampled embeddings, IDs and scores still line up
    for n, full in (("ids", ids), ("scores", sc)):
        assert np.array_equal(np.load(tmp_path / "s1" / f"{n}_rows.npy"), rows)
        assert np.array_equal(np.load(tmp_path / "s1" / f"{n}.npy"), full.numpy()[rows])
