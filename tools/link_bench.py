"""Linked centroid linkage (sdk_linked_linkage, csrc/ahc.hip's LINK kernels) on one MI355X -> one JSON line.

Rows look like per-recording centroids: d = 256 unit rows, recordings of 5 speakers drawn without repetition from a fixed pool of identities
(random unit vectors) plus gaussian noise; the group of a row is its recording.  Cases N = 2000, 10000, 50000 rows.  Per case, warm HIP-event
times of Engine.linked_linkage with stop = threshold and with stop = +inf, of Engine.centroid_linkage on the same rows (N <= 32000), the
distance + nearest-neighbour part alone (sdk_set_option "ahc_distances_only") and the merge kernel as the difference, the merges made and the
microseconds per merge; tests/link_ref.py's numpy restatement is timed and compared where it finishes in reasonable time (N <= 2000).
The no-regression figure: N = 10000, all groups -1, stop = +inf against sdk_centroid_linkage on the same input in the same run (a ratio).
    python tools/link_bench.py [--iters 3] [--sizes 2000,10000,50000] [--no-ref] [--out FILE]"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
PKG = "speaker-diarization-toolkit_amd"
REF_LIMIT_N = 2000
FREE_LIMIT_N = 32000
THRESHOLD = 0.7045654963945799
DIM, PER_REC, POOL, NOISE = 256, 5, 400, 0.25


def rows(N: int, seed: int):
    import numpy as np
    rng = np.random.default_rng(seed)
    pool = rng.standard_normal((POOL, DIM))
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)
    n_rec = -(-N // PER_REC)
    who = np.stack([rng.permutation(POOL)[:PER_REC] for _ in range(n_rec)]).reshape(-1)[:N]
    X = pool[who] + NOISE * rng.standard_normal((N, DIM)) / np.sqrt(DIM)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32), (np.arange(N) // PER_REC).astype(np.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sizes", default="2000,10000,50000")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    eng = ops.get_engine(0)

    def timed(fn, iters):
        fn()                                           # warm (code objects, allocator)
        torch.cuda.synchronize()
        ts, out = [], None
        for _ in range(iters):
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            out = fn()
            a1.record()
            torch.cuda.synchronize()
            ts.append(a0.elapsed_time(a1))
        return float(np.median(ts)), out

    out = {"bench": "linked_linkage", "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "dim": DIM, "threshold": THRESHOLD,
           "cases": []}
    for N in [int(s) for s in a.sizes.split(",") if s]:
        X, grp = rows(N, 1000 + N)
        E, G = torch.from_numpy(X).cuda(), torch.from_numpy(grp).cuda()
        iters = a.iters if N <= 10000 else 1
        eng.set_option("ahc_distances_only", 1)
        try:
            ms_dist, _ = timed(lambda: eng.linked_linkage(E, G, None, THRESHOLD), iters)
        finally:
            eng.set_option("ahc_distances_only", 0)
        rec = {"N": N, "recordings": int(grp[-1]) + 1, "dist_nn_ms": round(ms_dist, 3), "workspace_gb": round(N * N * 8 / 1e9, 3)}
        for name, stop in (("stop_threshold", THRESHOLD), ("stop_inf", None)):
            ms, (Z, m) = timed(lambda: eng.linked_linkage(E, G, None, stop), iters)
            merges = int(m.cpu()[0])
            rec[name] = {"gpu_ms": round(ms, 3), "merge_ms": round(ms - ms_dist, 3), "merges": merges,
                         "us_per_merge": round((ms - ms_dist) * 1e3 / max(merges, 1), 2)}
            if name == "stop_threshold":
                lab = importlib.import_module(f"{PKG}.cluster")._flat_partition(Z.cpu().numpy(), N, merges)
                rec[name]["clusters"] = int(lab.max()) + 1
                Zt = Z.cpu().numpy()
        if N <= FREE_LIMIT_N:
            ms, _ = timed(lambda: eng.centroid_linkage(E), iters)
            rec["centroid_linkage"] = {"gpu_ms": round(ms, 3), "merge_ms": round(ms - ms_dist, 3), "merges": N - 1,
                                       "us_per_merge": round((ms - ms_dist) * 1e3 / (N - 1), 2)}
        if not a.no_ref and N <= REF_LIMIT_N:
            import link_ref
            t0 = time.perf_counter()
            Zr, mr, _ = link_ref.linked_linkage(X, grp, THRESHOLD)
            rec["numpy_ref_s"] = round(time.perf_counter() - t0, 3)
            rec["equals_numpy_ref"] = bool(mr == rec["stop_threshold"]["merges"] and np.array_equal(Zt[:, [0, 1, 3]], Zr[:, [0, 1, 3]])
                                           and np.allclose(Zt[:, 2], Zr[:, 2], rtol=1e-12, atol=0))
        else:
            rec["numpy_ref_s"] = None
        if N == 10000:                                 # the no-regression figure: nothing forbidden, no stop, against the plain kernels
            free = torch.full((N,), -1, dtype=torch.int32, device="cuda")
            ms_l, (Zl, _) = timed(lambda: eng.linked_linkage(E, free, None, None), a.iters)
            ms_c, Zc = timed(lambda: eng.centroid_linkage(E), a.iters)
            out["no_regression_n10000"] = {"linked_ms": round(ms_l, 3), "centroid_ms": round(ms_c, 3), "ratio": round(ms_l / ms_c, 4),
                                           "bit_identical": bool(torch.equal(Zl, Zc))}
        out["cases"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del E, G, Z
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
