"""Centroid-linkage agglomerative clustering (sdk_centroid_linkage, csrc/ahc.hip) on one MI355X -> one JSON line.

Cases: single problems at N = 2000, 10000, 32000 and a batch of G = 64 problems of N ~ 1000 (192-d unit rows, oracle.spectral.vmf_mixture).
GPU times are warm, from HIP events around Engine.centroid_linkage's launch sequence; the distance + nearest-neighbour part is timed the same
way with sdk_set_option("ahc_distances_only", 1), and the merge kernel is the difference.  scipy.cluster.hierarchy.linkage(X, "centroid")
on the same float64 rows is timed on the host where it finishes in under a minute (larger N: skipped, not extrapolated).
Merge-kernel bytes are a lower bound from shapes: per merge of a problem of n rows with m live clusters, the nnd scan reads 12 n bytes
(nnd + liveness) and the Lance-Williams update reads rows x and y and writes row and column y (32 m bytes); rescans are not counted.
    python tools/ahc_bench.py [--iters 3] [--no-scipy] [--out FILE]"""
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
SCIPY_LIMIT_N = 12000          # scipy at 10k rows takes ~10 s here; at 32k it would take minutes


def merge_bytes(n: int) -> int:
    return sum(12 * n + 32 * (n - t) for t in range(n - 1))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--sizes", default="2000,10000,32000")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from oracle.spectral import vmf_mixture
    ops = importlib.import_module(f"{PKG}.ops")
    eng = ops.get_engine(0)

    def timed(E, off, iters):
        eng.centroid_linkage(E, off)                   # warm (code objects, allocator)
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            Z = eng.centroid_linkage(E, off)
            a1.record()
            torch.cuda.synchronize()
            ts.append(a0.elapsed_time(a1))
        return float(np.median(ts)), Z

    cases = [("single", [int(s)]) for s in a.sizes.split(",") if s]
    rng = np.random.default_rng(0)
    cases.append(("batch", [int(v) for v in rng.integers(950, 1051, size=a.batch)]))
    out = {"bench": "centroid_linkage", "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "cases": []}
    for kind, sizes in cases:
        X = np.concatenate([vmf_mixture(n, 192, 8, 1000 + i, 0.5)[0] for i, n in enumerate(sizes)])
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        E = eng.l2norm(torch.from_numpy(X).cuda())[0]
        iters = a.iters if max(sizes) > 5000 else 3 * a.iters
        ms, Z = timed(E, off, iters)
        eng.set_option("ahc_distances_only", 1)
        try:
            ms_dist, _ = timed(E, off, iters)
        finally:
            eng.set_option("ahc_distances_only", 0)
        mb = sum(merge_bytes(n) for n in sizes)
        ms_merge = ms - ms_dist
        rec = {"kind": kind, "G": len(sizes), "N": sizes[0] if kind == "single" else int(np.mean(sizes)), "N_total": int(off[-1]),
               "gpu_ms": round(ms, 3), "dist_nn_ms": round(ms_dist, 3), "merge_ms": round(ms_merge, 3),
               "workspace_gb": round(sum(n * n * 8 for n in sizes) / 1e9, 3),
               "merge_gb_lower_bound": round(mb / 1e9, 3),
               "merge_gbps_per_problem": round(mb / len(sizes) / (ms_merge * 1e-3) / 1e9, 1) if ms_merge > 0 else None}
        if not a.no_scipy and max(sizes) <= SCIPY_LIMIT_N:
            from scipy.cluster.hierarchy import linkage
            Eh = E.cpu().numpy().astype(np.float64)
            Zh = Z.cpu().numpy()
            t0 = time.perf_counter()
            same = True
            for g, n in enumerate(sizes):
                Zs = linkage(Eh[off[g]:off[g + 1]], "centroid")
                Zg = Zh[off[g] - g: off[g] - g + n - 1]
                same &= bool(np.array_equal(Zg[:, [0, 1, 3]], Zs[:, [0, 1, 3]]) and np.allclose(Zg[:, 2], Zs[:, 2], rtol=1e-12, atol=0))
            rec["scipy_s"] = round(time.perf_counter() - t0, 3)
            rec["speedup_vs_scipy"] = round(rec["scipy_s"] * 1e3 / ms, 1)
            rec["equals_scipy"] = same
        else:
            rec["scipy_s"] = None
        out["cases"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del E, Z
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
