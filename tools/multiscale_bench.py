"""The multi-scale form of clustering="nmesc" (cluster.nmesc_multiscale, ops_cluster.knn_rows_fused; sdk_knn_rows_fused in csrc/nmesc.hip) on
one MI355X -> one JSON line.

Generated unit rows (oracle.spectral.vmf_mixture) at n = 2 000 / 14 400 base rows (one hour at a 0.25-s hop), d = 256, with 2 / 4 planted
speakers, at S = 1 / 3 / 5 scales.  Scale s of S has hop ratio S - s (S = 3: 3, 2, 1; the base scale, last, is the identity): its row g
is the unit mean of base rows g r .. g r + r - 1, and maps[s][i] = that scale's offset + i // r.  Device times are HIP events around the
call, after two warm-up calls: the least of --windows windows, each the mean of --iters calls (tools/nmesc_bench.py's).  Per size:
`knn_rows_ms`, sdk_knn_rows on the n base rows alone, in the same process; per S: `fused_ms` (sdk_knn_rows_fused; the wrapper's status read is
inside both), `fused_over_rows` = fused_ms / knn_rows_ms, the figure to hold against S; `call_ms`, the whole nmesc_multiscale, wall clock,
beside `nmesc_cluster_ms`, the whole nmesc_cluster on the base rows; and the count found.
    python tools/multiscale_bench.py [--sizes 2000,14400] [--scales 1,3,5] [--iters 3] [--windows 3] [--out FILE]"""
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
PLANTED = {2000: 2, 14400: 4}


def stacked(np, base, S):
    """-> (E_all fp32 [n_all, d], maps int32 [S, n]) of S scales with hop ratios S, S - 1, .. 1 over the base rows."""
    n = base.shape[0]
    tables, maps, off = [], [], 0
    for r in range(S, 0, -1):
        g = (n + r - 1) // r
        rows = np.add.reduceat(base.astype(np.float64), np.arange(0, n, r), axis=0) if r > 1 else base.astype(np.float64)
        tables.append((rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32))
        maps.append(off + np.arange(n) // r)
        off += g
    return np.concatenate(tables), np.stack(maps).astype(np.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,14400")
    ap.add_argument("--scales", default="1,3,5")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from oracle.spectral import vmf_mixture
    ops = importlib.import_module(f"{PKG}.ops")
    cluster = importlib.import_module(f"{PKG}.cluster")
    OC = importlib.import_module(f"{PKG}.ops_cluster")
    eng = ops.get_engine(0)
    d = 256

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

    out = {"bench": "multiscale", "d": d, "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "iters": a.iters,
           "windows": a.windows, "sizes": {}}
    for n in (int(v) for v in a.sizes.split(",")):
        k = PLANTED.get(n, 4)
        Eh, lab = vmf_mixture(n, d, k, 0)
        order = np.argsort(lab, kind="stable")                        # a speaker's rows in one stretch, as in time: a coarse row then averages
        Eh, lab = np.ascontiguousarray(Eh[order]), cluster.canonical_labels(lab[order]).astype(lab.dtype)      # one speaker's rows
        E = torch.from_numpy(Eh).cuda()
        rec = {"planted": k, "knn_rows_ms": timed(lambda: OC.knn_rows(eng, E)), "nmesc_cluster_ms": wall(lambda: cluster.nmesc_cluster(eng, E)),
               "scales": {}}
        for S in (int(v) for v in a.scales.split(",")):
            Ea, maps = stacked(np, Eh, S)
            E_all, maps_d = torch.from_numpy(Ea).cuda(), torch.from_numpy(maps).cuda()
            w = [1.0 / S] * S
            ms = timed(lambda: OC.knn_rows_fused(eng, E_all, maps_d, w))
            res = cluster.nmesc_multiscale(eng, E_all, maps_d)
            rec["scales"][str(S)] = {"hop_ratios": list(range(S, 0, -1)), "n_all": int(Ea.shape[0]), "fused_ms": ms,
                                     "fused_over_rows": ms / rec["knn_rows_ms"],
                                     "call_ms": wall(lambda: cluster.nmesc_multiscale(eng, E_all, maps_d)), "p": res.p, "k": res.n_speakers,
                                     "labels_equal_planted": bool(np.array_equal(res.labels, lab)), "host_reads": res.host_reads}
        out["sizes"][str(n)] = rec
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
