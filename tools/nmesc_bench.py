"""Eigengap spectral clustering on the nearest-neighbour graph (clustering="nmesc": cluster.nmesc_cluster, ops_cluster.knn_rows .. knn_matvec;
csrc/nmesc.hip) on one MI355X -> one JSON line.

Generated unit rows (oracle.spectral.vmf_mixture) at n = 2 000 / 14 400 / 32 000, d = 256, with 2 / 4 / 8 planted speakers.  Device times
are HIP events around the call, after two warm-up calls: the least of --windows windows, each the mean of --iters calls.  Per size:
`knn_rows_ms` (product and selection are one kernel and are not split; the wrapper's status read is inside), `knn_reverse_ms`, one
`knn_matvec` at p = 8 and p = 64 on a [n, 24] block with its bytes (lists, reverse entries, dinv gathers, X gathers, Y) over the time as
a fraction of --hbm-gbs; `sweep_ms` per candidate (degrees, n_iter steps of mat-vec + CholeskyQR2, the Ritz step) with its library calls
(counted by entry point) and the launches computed from them; `final_ms` (the pass for p*: the same, then rows_apply, rows_unit and the k-means); `call_ms`, the whole nmesc_cluster, wall clock,
beside `linkage_ms`, Engine.centroid_linkage on the same rows; and, at n = 2 000 only, `host_s`, cluster.nmesc_host.
    python tools/nmesc_bench.py [--sizes 2000,14400,32000] [--iters 3] [--windows 3] [--hbm-gbs 8000] [--out FILE]"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
PLANTED = {2000: 2, 14400: 4, 32000: 8}
# kernels one call of each entry point of a sweep enqueues (read from csrc/: sdk_rows_gram is two-stage); a call of an entry point that is
# not listed here is a KeyError, so the computed launches cannot silently miss one
LAUNCHES_PER_CALL = {"sdk_knn_degree": 1, "sdk_knn_matvec": 1, "sdk_rows_gram": 2, "sdk_chol_inverse": 1, "sdk_rows_apply": 1, "sdk_sym_eigh": 1}


class _Tally:
    """The library with every call counted by name (size queries, *_workspace_bytes, launch nothing and are left out)."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith("_workspace_bytes"):
            return fn

        def call(*args):
            self._calls[name] = self._calls.get(name, 0) + 1
            return fn(*args)
        return call


def counted_calls(eng, fn) -> dict:
    """The library calls fn makes through eng, by entry point."""
    calls, lib = {}, eng.lib
    eng.lib = _Tally(lib, calls)
    try:
        fn()
    finally:
        eng.lib = lib
    return calls


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,14400,32000")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--no-linkage", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from oracle.spectral import vmf_mixture
    ops = importlib.import_module(f"{PKG}.ops")
    cluster = importlib.import_module(f"{PKG}.cluster")
    OC = importlib.import_module(f"{PKG}.ops_cluster")
    eng = ops.get_engine(0)
    d, kv = 256, 24

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / a.iters)
        return best

    out = {"bench": "nmesc", "d": d, "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "iters": a.iters,
           "windows": a.windows, "hbm_gbs_assumed": a.hbm_gbs, "sizes": {}}
    for n in (int(v) for v in a.sizes.split(",")):
        k = PLANTED.get(n, 4)
        Eh, lab = vmf_mixture(n, d, k, 0)
        E = torch.from_numpy(Eh).cuda()
        rec = {"planted": k}
        rec["knn_rows_ms"] = timed(lambda: OC.knn_rows(eng, E))
        idx, _ = OC.knn_rows(eng, E)
        rec["knn_reverse_ms"] = timed(lambda: OC.knn_reverse(eng, idx, check_idx=False))
        rev = OC.knn_reverse(eng, idx)
        X = torch.randn((n, kv), device="cuda")
        P = min(64, n - 1)
        for p in (8, 64):
            _, dinv = OC.knn_degree(eng, rev[0], rev[2], P, p)
            ms = timed(lambda: OC.knn_matvec(eng, idx, rev, dinv, p, X))
            edges = 2.0 * n * p                                     # out-entries read, and as many reverse entries of rank < p
            nbytes = 4.0 * n * p + 8.0 * n * P + edges * (8.0 + 4.0 * kv) + 8.0 * n * kv
            rec[f"matvec_p{p}_ms"] = ms
            rec[f"matvec_p{p}_hbm_fraction"] = nbytes / (ms * 1e-3) / (a.hbm_gbs * 1e9)
        ps = cluster.nmesc_candidates(n)
        m, b = cluster._nmesc_shape(n, cluster.NMESC_MAX_COUNT)
        V0 = torch.randn((n, b), device="cuda")
        comm, flag = cluster._Comm(single=True), torch.zeros((1,), dtype=torch.int32, device="cuda")

        def ritz(p):
            _, dinv = OC.knn_degree(eng, rev[0], rev[2], P, p)
            V = cluster._orth(eng, comm, V0, b, flag)
            for _ in range(cluster.NMESC_N_ITER):
                V = cluster._orth(eng, comm, OC.knn_matvec(eng, idx, rev, dinv, p, V), b, flag)
            return V, eng.sym_eigh(eng.rows_gram(V, OC.knn_matvec(eng, idx, rev, dinv, p, V)))
        rec["sweep_ms_per_candidate"] = {str(p): timed(lambda: ritz(p)) for p in ps}
        calls = counted_calls(eng, lambda: ritz(ps[0]))
        rec["sweep_library_calls_per_candidate"] = calls                         # counted: one sweep with every library call tallied
        rec["sweep_launches_per_candidate_computed"] = sum(c * LAUNCHES_PER_CALL[name] for name, c in calls.items())

        def final(p, kk):
            V, (Q, _) = ritz(p)
            U = eng.rows_apply(V, Q)[:, :kk].contiguous()
            return cluster._kmeans(eng, comm, eng.rows_unit(U), 0, n, kk, cluster.NMESC_KMEANS_PASSES)
        res = cluster.nmesc_cluster(eng, E)
        rec.update(p=res.p, k=res.n_speakers, labels_equal_planted=bool(np.array_equal(res.labels, lab)), host_reads=res.host_reads)
        rec["final_ms"] = timed(lambda: final(res.p, max(res.n_speakers, 2)))

        def wall(fn):
            fn()
            best = float("inf")
            for _ in range(a.windows):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t)
            return best * 1e3
        rec["call_ms"] = wall(lambda: cluster.nmesc_cluster(eng, E))
        if not a.no_linkage:
            rec["linkage_ms"] = wall(lambda: eng.centroid_linkage(E))
        if n <= 2000:
            t = time.perf_counter()
            host = cluster.nmesc_host(Eh)
            rec["host_s"] = time.perf_counter() - t
            rec["host_equals_device"] = bool(host.p == res.p and host.n_speakers == res.n_speakers and np.array_equal(host.labels, res.labels))
            rec["eigenvalue_worst_deviation_first_k"] = float(np.abs(host.eigenvalues[:, :k] - res.eigenvalues[:, :k]).max())
        out["sizes"][str(n)] = rec
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
