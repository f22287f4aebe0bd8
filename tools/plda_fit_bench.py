#!/usr/bin/env python3
"""Device time of the PLDA training's passes (plda.fit: sdk_plda_fit_stats, sdk_plda_project) beside a torch float64 yardstick and the host solves.

N in {2^20, 2^16} labelled rows, d_in = 256, D0 = 128, K = 8192 classes.  Each pass is timed with device events around the one call (all launches
enqueued, no host synchronisation inside; the label sort is torch's and is inside the call), --warmup calls first, then --repeats calls: the
median and the minimum are reported.

  mean_ms, stats1_ms, project_ms, stats2_ms   the four passes over the rows
  scatter_ms                                  stats1 with the scatter minus stats1 without it: the f64 MFMA kernel and its finish
  scatter_fraction_of_fp64_matrix_peak        2 N d^2 flop / scatter_ms over FP64_MATRIX_PEAK (the datasheet's 78.6 TFLOP/s of the MI355X;
                                              only the upper triangle of macro tiles is computed: the rate is of the full product)
  torch_xtx_ms, torch_index_add_ms            the yardstick on the same materialised float64 rows x1: X.T @ X, and index_add_ into [K, d]
  host_solve_ms                               plda.fit_from_stats on the downloaded statistics (numpy, at most 16 threads), without the passes

Prints one JSON line; the record is profiles/r28_plda_fit_bench.json."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))
import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
FP64_MATRIX_PEAK = 78.6e12


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 20, 1 << 16])
    ap.add_argument("--d-in", type=int, default=256)
    ap.add_argument("--D0", type=int, default=128)
    ap.add_argument("--classes", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    lib = importlib.import_module(f"{PKG}._lib")
    P = importlib.import_module(f"{PKG}.plda")
    eng = ops.get_engine(0)
    d, D0, K = args.d_in, args.D0, args.classes

    def timed(call):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(min(ts))

    out = {"tool": "plda_fit_bench", "device": lib.device_info(0)["name"], "d_in": d, "D0": D0, "K": K, "warmup": args.warmup, "repeats": args.repeats,
           "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "cases": []}
    for N in args.rows:
        g = torch.Generator(device="cuda").manual_seed(N)
        means = torch.randn((K, d), generator=g, device="cuda") * torch.linspace(3.0, 0.3, d, device="cuda")
        labels = torch.randint(0, K, (N,), generator=g, device="cuda", dtype=torch.int32)
        labels[:K] = torch.arange(K, dtype=torch.int32, device="cuda")
        E = means[labels.long()] + torch.randn((N, d), generator=g, device="cuda")
        E = (E / E.norm(dim=1, keepdim=True)).contiguous()
        mean1 = eng.plda_fit_stats(E, scatter=False)["total"] / N
        s1 = eng.plda_fit_stats(E, labels, K, mean1=mean1, check_labels=False)
        host = {k: s1[k].cpu().numpy() for k in ("counts", "sums", "total", "scatter")}
        keep = {}

        def stats2(m1, lda, mean2):
            keep["lda"], keep["mean2"] = torch.from_numpy(lda).cuda(), torch.from_numpy(mean2).cuda()
            X2 = eng.plda_project(E, mean1, keep["lda"], keep["mean2"])
            keep["X2"] = X2
            return {k: v.cpu().numpy() for k, v in eng.plda_fit_stats(X2, labels, K, check_labels=False).items() if k != "status"}

        t0 = time.perf_counter()
        model, fit = P.fit_from_stats((mean1 * N).cpu().numpy(), lambda m1: host, stats2, N, D0, 128 if D0 >= 128 else 64, 10)
        t_fit = time.perf_counter() - t0
        t0 = time.perf_counter()
        stats2(None, model.lda, model.mean2)
        torch.cuda.synchronize()
        t_pass = time.perf_counter() - t0
        ms = {"mean": timed(lambda: eng.plda_fit_stats(E, scatter=False)),
              "stats1": timed(lambda: eng.plda_fit_stats(E, labels, K, mean1=mean1, check_labels=False)),
              "stats1_no_scatter": timed(lambda: eng.plda_fit_stats(E, labels, K, mean1=mean1, scatter=False, check_labels=False)),
              "project": timed(lambda: eng.plda_project(E, mean1, keep["lda"], keep["mean2"])),
              "stats2": timed(lambda: eng.plda_fit_stats(keep["X2"], labels, K, check_labels=False))}
        # the yardstick: the same rows x1, materialised in float64
        X1 = (E.double() - mean1) * (float(np.sqrt(d)) / (E.double() - mean1).norm(dim=1, keepdim=True))
        lab64 = labels.long()
        acc = torch.zeros((K, d), dtype=torch.float64, device="cuda")
        ms["torch_xtx"] = timed(lambda: X1.T @ X1)
        ms["torch_index_add"] = timed(lambda: acc.zero_().index_add_(0, lab64, X1))
        rel = float(((X1.T @ X1) - s1["scatter"]).abs().max() / s1["scatter"].abs().max())
        scat = ms["stats1"][0] - ms["stats1_no_scatter"][0]
        case = {"N": N, **{f"{k}_ms": round(v[0], 4) for k, v in ms.items()}, **{f"{k}_ms_min": round(v[1], 4) for k, v in ms.items()},
                "scatter_ms": round(scat, 4), "scatter_tflops": round(2.0 * N * d * d / (scat * 1e-3) / 1e12, 3),
                "scatter_fraction_of_fp64_matrix_peak": round(2.0 * N * d * d / (scat * 1e-3) / FP64_MATRIX_PEAK, 4),
                "torch_xtx_tflops": round(2.0 * N * d * d / (ms["torch_xtx"][0] * 1e-3) / 1e12, 3),
                "host_solve_ms": round((t_fit - t_pass) * 1e3, 1), "scatter_rel_diff_to_torch": rel, "objf_first_last": [float(fit.objf[0]), float(fit.objf[-1])],
                "n_classes": fit.n_classes}
        out["cases"].append(case)
        del X1, E, acc, keep, s1
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
