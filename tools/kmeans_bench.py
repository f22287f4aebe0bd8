"""Spherical k-means on unit rows (sdk_kmeans_rows; csrc/kmeans.hip) on one MI355X -> one JSON line.

N = 14 400 and 65 536 planted unit rows, d = 256, k = 2, 8, 64.  Device times are warm medians from HIP events around Engine.kmeans_rows (the
whole enqueue: seeding and every iteration): `call_ms` with cluster.KMEANS_MAX_ITERS, n_iter from the one read, and `iter_ms` = (the call
with max_iters = n_iter minus the call with max_iters = 1) / (n_iter - 1): one assignment + one update.  The torch yardstick is one Lloyd
iteration on the same rows in float64 (E @ C.T, argmax, index_add_, normalise); the numpy restatement (tests/kmeans_ref.py, sums in the
stated order) is timed at the smaller N only, per iteration.  `diarize`: Diarizer.run on tools/diarize_bench.py's synthetic recording
(--seconds, default the hour) with clustering="vbx", wall clock, with and without speakers=k forcing the k-means; `share` is what it adds.
    python tools/kmeans_bench.py [--iters 10] [--seconds 3600] [--no-diarize] [--out FILE]"""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--no-diarize", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import kmeans_ref as KR
    ops = importlib.import_module(f"{PKG}.ops")
    cluster = importlib.import_module(f"{PKG}.cluster")
    eng = ops.get_engine(0)
    d = 256

    def timed(fn, iters=a.iters):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    def planted(N, k, seed=0, noise=3.0):
        rng = np.random.default_rng(seed)
        cen = rng.standard_normal((k, d))
        cen /= np.linalg.norm(cen, axis=1, keepdims=True)
        X = cen[rng.integers(0, k, N)] + noise * rng.standard_normal((N, d)) / np.sqrt(d)
        return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)

    out = {"bench": "kmeans_rows", "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "d": d, "iters": a.iters,
           "max_iters": cluster.KMEANS_MAX_ITERS, "cases": []}
    for N in (14400, 65536):
        for k in (2, 8, 64):
            Eh = planted(N, k)
            E = torch.from_numpy(Eh).cuda()
            rows = torch.arange(N, dtype=torch.int32, device="cuda")
            _, n_iter, status = eng.kmeans_rows(E, rows, k, cluster.KMEANS_MAX_ITERS)
            n_it = int(n_iter.item())
            assert int(status.item()) == 0
            call_ms = timed(lambda: eng.kmeans_rows(E, rows, k, cluster.KMEANS_MAX_ITERS))
            one_ms = timed(lambda: eng.kmeans_rows(E, rows, k, 1))
            run_ms = timed(lambda: eng.kmeans_rows(E, rows, k, n_it)) if n_it > 1 else one_ms
            E64 = E.double()
            C = E64[:k].clone()

            def torch_iter():
                lab = (E64 @ C.T).argmax(dim=1)
                s = torch.zeros((k, d), dtype=torch.float64, device="cuda").index_add_(0, lab, E64)
                return s / s.norm(dim=1, keepdim=True).clamp_min(1e-300)

            case = {"N": N, "k": k, "n_iter": n_it, "call_ms": round(call_ms, 4), "seed_and_first_assign_ms": round(one_ms, 4),
                    "iter_ms": round((run_ms - one_ms) / (n_it - 1), 4) if n_it > 1 else None, "torch_iter_ms": round(timed(torch_iter), 4)}
            if case["iter_ms"]:
                case["torch_over_kernel_per_iter"] = round(case["torch_iter_ms"] / case["iter_ms"], 2)
            if N == 14400:
                t0 = time.perf_counter()
                ref = KR.kmeans(Eh, k, max_iters=2)
                case["numpy_restatement_iter_ms"] = round((time.perf_counter() - t0) * 1e3 / ref["n_iter"], 1)
            out["cases"].append(case)
    if not a.no_diarize:
        seg = importlib.import_module(f"{PKG}.segmentation")
        rn = importlib.import_module(f"{PKG}.resnet")
        dz = importlib.import_module(f"{PKG}.diarize")
        n = int(a.seconds * 16000)
        rng = np.random.default_rng(0)
        x = np.clip(np.round(rng.normal(0, 0.1, n) * (1 + np.sin(2 * np.pi * 0.3 * np.arange(n) / 16000)) * 32768), -32768, 32767).astype(np.int16)
        dia = dz.Diarizer(eng, seg.Segmentation(eng, seg.synthetic_weights(0)), rn.ResNet34(eng, rn.synthetic_weights(0)))
        kw = dict(step_s=1.0, threshold=cluster.VBX_AHC_THRESHOLD, clustering="vbx")

        def wall(**more):
            best, res = None, None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = dia.run(x, **kw, **more)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            return best, res

        t_free, free = wall()
        k = 2 if free.n_speakers != 2 else 3
        t_k, forced = wall(speakers=k)
        out["diarize"] = {"seconds": a.seconds, "clustering": "vbx", "found": free.n_speakers, "speakers": k, "forced": forced.forced,
                          "run_s": round(t_free, 4), "run_speakers_s": round(t_k, 4), "share": round((t_k - t_free) / t_k, 4)}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
