"""Verification trials (sdk_trial_hist; csrc/trials.hip) on one MI355X -> one JSON line.

N = M rows of K columns (unit rows in float64, the cosine form), ~1000 speakers, sessions 0 .. 63.  Per case, device times from HIP events
(every variant is called once untimed first; then the median of --iters calls up to --small rows and of a quarter as many above; the
two kernel variants alternate call by call, so a drift of the clock meets both):
  pass1_ms / zoom_ms            Engine.trial_hist at (12, 0) and at (0, 4096 b), b the busiest coarse bin
  product_tflops / fraction     2 N M K / pass1 time, against the 78.6 TFLOP/s fp64 matrix peak
  nohist_*_ms                   the same kernel with the epilogue's LDS atomics compiled out (sdk_set_option "trials_no_hist"): what the
                                histogram costs is the difference
  torch_ms                      the yardstick on the same tensors: row blocks of float64 A_blk @ B.T + r, the same q arithmetic, the class
                                and exclusion masks and torch.bincount per block
The yardstick's product rounds differently from the kernel's, so a handful of trials within an ulp of a cell edge may land in a neighbouring
bin: `torch_max_cum_diff` is the largest difference of the cumulative counts (reported, not asserted; tests/test_trials_gpu.py pins the kernel).
    python tools/trials_bench.py [--sizes 16384,65536] [--ks 192,256] [--iters 20] [--small 16384] [--out FILE]"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
FP64_MATRIX_TFLOPS = 78.6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--ks", default="192,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--small", type=int, default=16384)
    ap.add_argument("--speakers", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    trials = importlib.import_module(f"{PKG}.trials")
    eng = ops.get_engine(0)
    lo, hi = trials.COSINE_RANGE
    scale = trials.scale_of(lo, hi)
    g = torch.Generator(device="cuda").manual_seed(0)

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), got

    def timed(fn, iters):
        fn()
        torch.cuda.synchronize()
        return float(np.median([one(fn)[0] for _ in range(iters)]))

    def timed_ab(fn, iters):
        """fn(flag) with the LDS atomics (flag 0) and without (flag 1), alternating -> the two medians."""
        ts = ([], [])
        for it in range(iters + 1):
            for flag in (0, 1):
                eng.set_option("trials_no_hist", flag)
                try:
                    ms, _ = one(lambda: fn())
                finally:
                    eng.set_option("trials_no_hist", 0)
                if it:                               # the first round is the warm-up
                    ts[flag].append(ms)
        return float(np.median(ts[0])), float(np.median(ts[1]))

    out = {"bench": "trials", "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "speakers": a.speakers,
           "score_range": [lo, hi], "fp64_matrix_peak_tflops": FP64_MATRIX_TFLOPS, "cases": []}
    for K in [int(s) for s in a.ks.split(",") if s]:
        for N in [int(s) for s in a.sizes.split(",") if s]:
            M = N
            iters = a.iters if N <= a.small else max(3, a.iters // 4)

            def rows(n):
                X = torch.randn((n, K), generator=g, device="cuda", dtype=torch.float64)
                return (X / X.norm(dim=1, keepdim=True)).contiguous()

            A, B = rows(N), rows(M)
            r = torch.zeros((M,), dtype=torch.float64, device="cuda")
            la, lb = (torch.randint(0, a.speakers, (n,), generator=g, device="cuda", dtype=torch.int32) for n in (N, M))
            sa, sb = (torch.randint(0, 64, (n,), generator=g, device="cuda", dtype=torch.int32) for n in (N, M))

            def run(shift, base):
                return eng.trial_hist(A, B, r, la, sa, lb, sb, lo, hi, shift=shift, base=base)

            coarse = trials.counts_to_host(run(12, 0))
            b = int(np.argmax(coarse.hist.sum(axis=0)))
            pass1_ms, nh1_ms = timed_ab(lambda: run(12, 0), iters)
            zoom_ms, nhz_ms = timed_ab(lambda: run(0, 4096 * b), iters)
            print(f"trials_bench: N=M={N} K={K}: pass1 {pass1_ms:.2f} ms, zoom {zoom_ms:.2f} ms, without atomics {nh1_ms:.2f} / {nhz_ms:.2f} ms",
                  file=sys.stderr, flush=True)

            blk = 2048 if N <= 16384 else 1024
            la64, lb64, sa64, sb64 = la.long(), lb.long(), sa.long(), sb.long()

            def torch_pass():
                hist = torch.zeros(2 * 4096 + 6, dtype=torch.int64, device="cuda")       # hist, then under[2], over[2], nan[2]
                excluded = torch.zeros((), dtype=torch.int64, device="cuda")
                for i0 in range(0, N, blk):
                    S = A[i0:i0 + blk] @ B.T + r[None, :]
                    t = (S - lo) * scale
                    li, si = la64[i0:i0 + blk, None], sa64[i0:i0 + blk, None]
                    excl = (li < 0) | (lb64[None, :] < 0) | ((si >= 0) & (si == sb64[None, :]))
                    cls = (li == lb64[None, :]).long()
                    nan = t != t
                    q = t.clamp(0, 16777215).long() >> 12
                    slot = torch.where(nan, 8196 + cls, torch.where(t < 0, 8192 + cls, torch.where(t >= 16777216.0, 8194 + cls, cls * 4096 + q)))
                    hist += torch.bincount(slot[~excl], minlength=8198)
                    excluded += excl.sum()
                return hist, excluded

            th, te = torch_pass()
            torch_ms = timed(torch_pass, max(3, iters // 4))
            th = th.cpu().numpy()
            cum_dev = np.cumsum(coarse.hist, axis=1) + coarse.under[:, None]
            cum_t = np.cumsum(th[:8192].reshape(2, 4096), axis=1) + th[8192:8194][:, None]
            flops = 2.0 * N * M * K
            tf = flops / (pass1_ms * 1e-3) / 1e12
            out["cases"].append({
                "N": N, "M": M, "K": K, "iters": iters, "trials": N * M, "n_target": int(coarse.hist[1].sum() + coarse.under[1] + coarse.over[1]),
                "n_excluded": int(coarse.excluded), "busiest_bin": b, "busiest_bin_trials": int(coarse.hist[:, b].sum()),
                "pass1_ms": round(pass1_ms, 3), "zoom_ms": round(zoom_ms, 3), "product_tflops": round(tf, 2),
                "fraction_of_fp64_matrix_peak": round(tf / FP64_MATRIX_TFLOPS, 4), "nohist_pass1_ms": round(nh1_ms, 3), "nohist_zoom_ms": round(nhz_ms, 3),
                "histogram_share_of_pass1": round((pass1_ms - nh1_ms) / pass1_ms, 4),
                "histogram_share_of_zoom": round((zoom_ms - nhz_ms) / zoom_ms, 4), "torch_ms": round(torch_ms, 3),
                "speedup_vs_torch": round(torch_ms / pass1_ms, 2), "torch_excluded_equal": bool(int(te.item()) == coarse.excluded),
                "torch_max_cum_diff": int(np.abs(cum_dev - cum_t).max())})
            del A, B
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
