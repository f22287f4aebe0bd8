"""AS-norm verification trials (sdk_trial_hist_snorm; csrc/trials_snorm.hip) on one MI355X -> one JSON line.

N = M unit rows of K columns in float64 around ~1000 speaker centres, sessions 0 .. 63; per row a cohort mean near 0.15 and a reciprocal
standard deviation between 20 and 40 (generated: the bench measures the pass, not Engine.cohort_stats).  Per case, device times from HIP
events (every variant is called once untimed first; then the median of --iters calls up to --small rows and of a quarter as many above; the
variants alternate call by call, so a drift of the clock meets all of them):
  snorm_ms                      pass 1 of ops_score.trial_hist_snorm over trials_snorm.SNORM_RANGE
  hist_ms / snorm_over_hist     Engine.trial_hist (12, 0) on the same A, B (r = 0, the cosine range): the yardstick - what the six float64
                                operations per trial and the four staged statistics cost over the plain histogram.  A figure to report
  bilinear_ms                   K = 192 only: the same z as ONE product of width 2 K + 16 = 400 through Engine.trial_hist,
                                A' = [inv_a a / 2 | a / 2 | -mean_a inv_a / 2, 1 / 2, 0 ..], B' = [b | inv_b b | 1, -mean_b inv_b, 0 ..] - the matrix
                                form that needs no new kernel (and does not fit K <= 512 for the 256-wide families)
  torch_ms                      row blocks of float64 A_blk @ B.T, the same z and q arithmetic, the masks and torch.bincount per block
`torch_max_cum_diff` / `bilinear_max_cum_diff`: the largest difference of the cumulative counts against the kernel's (reported, not asserted:
the other two round differently; tests/test_trials_snorm_gpu.py pins the kernel).
    python tools/snorm_trials_bench.py [--sizes 16384,65536] [--ks 192,256] [--iters 20] [--small 16384] [--out FILE]"""
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
    ops_score = importlib.import_module(f"{PKG}.ops_score")
    trials = importlib.import_module(f"{PKG}.trials")
    ts = importlib.import_module(f"{PKG}.trials_snorm")
    eng = ops.get_engine(0)
    lo, hi = ts.SNORM_RANGE
    scale = trials.scale_of(lo, hi)
    clo, chi = trials.COSINE_RANGE
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

    def timed_round_robin(fns, iters):
        """The variants alternating call by call -> their medians (the first round is the warm-up)."""
        times = [[] for _ in fns]
        for it in range(iters + 1):
            for k, fn in enumerate(fns):
                ms, _ = one(fn)
                if it:
                    times[k].append(ms)
        return [float(np.median(t)) for t in times]

    def cumulative(p):
        return np.cumsum(p.hist, axis=1) + p.under[:, None]

    out = {"bench": "snorm_trials", "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "speakers": a.speakers,
           "score_range": [lo, hi], "fp64_matrix_peak_tflops": FP64_MATRIX_TFLOPS, "cases": []}
    for K in [int(s) for s in a.ks.split(",") if s]:
        centres = torch.randn((a.speakers, K), generator=g, device="cuda", dtype=torch.float64)
        for N in [int(s) for s in a.sizes.split(",") if s]:
            M = N
            iters = a.iters if N <= a.small else max(3, a.iters // 4)
            la, lb = (torch.randint(0, a.speakers, (n,), generator=g, device="cuda", dtype=torch.int32) for n in (N, M))
            sa, sb = (torch.randint(0, 64, (n,), generator=g, device="cuda", dtype=torch.int32) for n in (N, M))

            def rows(labels):
                X = centres[labels.long()] + 3.0 * torch.randn((len(labels), K), generator=g, device="cuda", dtype=torch.float64)
                return (X / X.norm(dim=1, keepdim=True)).contiguous()

            def stats(n):
                mean = 0.15 + 0.02 * torch.randn((n,), generator=g, device="cuda", dtype=torch.float64)
                inv = 20.0 + 20.0 * torch.rand((n,), generator=g, device="cuda", dtype=torch.float64)
                return mean.contiguous(), inv.contiguous()

            A, B = rows(la), rows(lb)
            (ma, ia), (mb, ib) = stats(N), stats(M)
            r = torch.zeros((M,), dtype=torch.float64, device="cuda")
            fns = [lambda: ops_score.trial_hist_snorm(eng, A, B, ma, ia, mb, ib, la, sa, lb, sb, lo, hi),
                   lambda: eng.trial_hist(A, B, r, la, sa, lb, sb, clo, chi)]
            if K == 192:
                pad = torch.zeros((N, 14), dtype=torch.float64, device="cuda")
                half = torch.full((N, 1), 0.5, dtype=torch.float64, device="cuda")
                A2 = torch.cat([0.5 * ia[:, None] * A, 0.5 * A, (-0.5 * ma * ia)[:, None], half, pad], dim=1).contiguous()
                B2 = torch.cat([B, ib[:, None] * B, torch.ones((M, 1), dtype=torch.float64, device="cuda"), (-mb * ib)[:, None], pad], dim=1).contiguous()
                assert A2.shape[1] == 2 * K + 16 == B2.shape[1]
                fns.append(lambda: eng.trial_hist(A2, B2, r, la, sa, lb, sb, lo, hi))
            coarse = trials.counts_to_host(fns[0]())
            ms = timed_round_robin(fns, iters)
            snorm_ms, hist_ms = ms[0], ms[1]
            print(f"snorm_trials_bench: N=M={N} K={K}: snorm {snorm_ms:.2f} ms, trial_hist {hist_ms:.2f} ms"
                  + (f", bilinear width {2 * K + 16}: {ms[2]:.2f} ms" if K == 192 else ""), file=sys.stderr, flush=True)

            blk = 2048 if N <= 16384 else 1024
            la64, lb64, sa64, sb64 = la.long(), lb.long(), sa.long(), sb.long()

            def torch_pass():
                hist = torch.zeros(2 * 4096 + 6, dtype=torch.int64, device="cuda")       # hist, then under[2], over[2], nan[2]
                excluded = torch.zeros((), dtype=torch.int64, device="cuda")
                for i0 in range(0, N, blk):
                    S = A[i0:i0 + blk] @ B.T
                    z = ((S - ma[i0:i0 + blk, None]) * ia[i0:i0 + blk, None] + (S - mb[None, :]) * ib[None, :]) * 0.5
                    t = (z - lo) * scale
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
            cum_t = np.cumsum(th[:8192].reshape(2, 4096), axis=1) + th[8192:8194][:, None]
            tf = 2.0 * N * M * K / (snorm_ms * 1e-3) / 1e12
            case = {"N": N, "M": M, "K": K, "iters": iters, "trials": N * M,
                    "n_target": int(coarse.hist[1].sum() + coarse.under[1] + coarse.over[1]), "n_excluded": int(coarse.excluded),
                    "n_outside_range": int(coarse.under.sum() + coarse.over.sum()), "snorm_ms": round(snorm_ms, 3), "hist_ms": round(hist_ms, 3),
                    "snorm_over_hist": round(snorm_ms / hist_ms, 4), "product_tflops": round(tf, 2),
                    "fraction_of_fp64_matrix_peak": round(tf / FP64_MATRIX_TFLOPS, 4), "torch_ms": round(torch_ms, 3),
                    "speedup_vs_torch": round(torch_ms / snorm_ms, 2), "torch_excluded_equal": bool(int(te.item()) == coarse.excluded),
                    "torch_max_cum_diff": int(np.abs(cumulative(coarse) - cum_t).max())}
            if K == 192:
                bil = trials.counts_to_host(fns[2]())
                case.update({"bilinear_width": 2 * K + 16, "bilinear_ms": round(ms[2], 3), "bilinear_over_snorm": round(ms[2] / snorm_ms, 3),
                             "bilinear_max_cum_diff": int(np.abs(cumulative(coarse) - cumulative(bil)).max())})
                del A2, B2
            out["cases"].append(case)
            del A, B
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
