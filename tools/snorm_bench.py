"""Adaptive score normalisation (sdk_cohort_stats, sdk_affinity_topk_snorm; csrc/snorm.hip) on one MI355X -> one JSON line.

N = 1000 windows, Pn = 100 profiles, K = 300, d = 192, cohorts of M = 2000, 10000, 100000 unit rows.  Device times are warm medians from HIP
events: Engine.cohort_stats (scoring + selection), the scoring kernel alone (sdk_set_option "snorm_scores_only"; its rate against the 155 TF
fp32 matrix rate), the selection as the difference, and Engine.affinity_topk_snorm.  The torch yardstick runs on the same tensors:
E @ C.T, torch.topk(K), mean and population std, and for the top-k Z = ... from a second matmul and torch.topk(1).  The identify step is
the embedding of 1000 two-second windows plus the raw affinity_topk (what identify_speaker runs without a cohort); `share` is what the
normalised path (window statistics + normalised top-1) adds to it.  Profile statistics are computed once per ProfileBatch and not counted.
    python tools/snorm_bench.py [--iters 20] [--sizes 2000,10000,100000] [--out FILE]"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
FP32_MATRIX_TFLOPS = 155.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="2000,10000,100000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    eng = ops.get_engine(0)
    N, Pn, K, d = 1000, 100, 300, 192
    g = torch.Generator(device="cuda").manual_seed(0)

    def unit_rows(n):
        return eng.l2norm(torch.randn((n, d), generator=g, device="cuda"))

    def timed(fn, iters=a.iters):
        for _ in range(3):
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

    E, Eb, re = unit_rows(N)
    P, Pb, rp = unit_rows(Pn)
    rpm = rp.max().reshape(1)
    pcm = (torch.randn((N, 32000), generator=g, device="cuda") * 3000).to(torch.int16)

    def identify_step():
        e, eb, r = eng.embed_pcm(pcm)
        eng.affinity_topk(e, eb, r, P, Pb, rpm, k=1)

    step_ms = timed(identify_step, max(3, a.iters // 4))
    out = {"bench": "snorm", "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "N": N, "Pn": Pn, "K": K, "d": d,
           "iters": a.iters, "identify_step_ms": round(step_ms, 4), "cases": []}
    for M in [int(s) for s in a.sizes.split(",") if s]:
        Cn = unit_rows(M)[0]
        ws = torch.empty(eng.lib.sdk_cohort_stats_workspace_bytes(N, M, K), dtype=torch.uint8, device="cuda")
        mean_p, std_p = eng.cohort_stats(P, Cn, K)
        mean_e, std_e = eng.cohort_stats(E, Cn, K, ws=ws)
        stats_ms = timed(lambda: eng.cohort_stats(E, Cn, K, ws=ws))
        eng.set_option("snorm_scores_only", 1)
        try:
            scores_ms = timed(lambda: eng.cohort_stats(E, Cn, K, ws=ws))
        finally:
            eng.set_option("snorm_scores_only", 0)
        topk_ms = timed(lambda: eng.affinity_topk_snorm(E, mean_e, std_e, P, mean_p, std_p, k=1))

        def torch_stats():
            top = torch.topk(E @ Cn.T, K, dim=1).values
            return top.mean(dim=1), top.std(dim=1, unbiased=False).clamp_min(1e-6)

        def torch_topk():
            S = E @ P.T
            Z = 0.5 * ((S - mean_e[:, None]) / std_e[:, None] + (S - mean_p[None, :]) / std_p[None, :])
            return torch.topk(Z, 1, dim=1)

        tm, ts_ = torch_stats()
        torch.cuda.synchronize()
        t_stats_ms, t_topk_ms = timed(torch_stats), timed(torch_topk)
        flops = 2.0 * N * M * d
        tf = flops / (scores_ms * 1e-3) / 1e12
        out["cases"].append({
            "M": M, "workspace_bytes": int(ws.numel()), "cohort_stats_ms": round(stats_ms, 4), "scoring_ms": round(scores_ms, 4),
            "selection_ms": round(stats_ms - scores_ms, 4), "scoring_tflops": round(tf, 2), "fraction_of_fp32_matrix_rate": round(tf / FP32_MATRIX_TFLOPS, 4),
            "affinity_topk_snorm_ms": round(topk_ms, 4), "torch_stats_ms": round(t_stats_ms, 4), "torch_topk_ms": round(t_topk_ms, 4),
            "speedup_stats_vs_torch": round(t_stats_ms / stats_ms, 2), "speedup_topk_vs_torch": round(t_topk_ms / topk_ms, 2),
            "max_abs_mean_diff_vs_torch": float((tm - mean_e).abs().max()), "max_abs_std_diff_vs_torch": float((ts_ - std_e).abs().max()),
            "share_of_identify_step": round((stats_ms + topk_ms) / step_ms, 4)})
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
