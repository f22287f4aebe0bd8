"""Calibration passes (sdk_trial_calib; csrc/trials.hip) on one MI355X -> one JSON line.

N = M unit rows of K columns in float64 (the cosine form) around ~1000 speaker centres, so that the target scores lie above the nontarget
ones and overlap with them; sessions 0 .. 63.  Per case, device times from HIP events (every variant is called once untimed first; then the
median of --iters calls up to --small rows and of a quarter as many above; the calibration pass and the histogram pass alternate call by
call, so a drift of the clock meets both):
  calib_ms / hist_ms / ratio    one ops_score.trial_calib pass at (a, c) = (8, -2) beside one Engine.trial_hist pass (12, 0) on the same tensors:
                                what the epilogue's double-precision exp, log1p and two divisions cost per trial over the histogram's integer
                                epilogue.  The ratio is the figure to report, not a target
  fit_passes / fit_wall_ms      trials.calibrate_scores end to end: pass 1, the zooms, every calibration pass and the host between them
                                (wall clock, one run after one untimed run)
  torch_ms                      the yardstick on the same tensors: row blocks of float64 A_blk @ B.T + r, the same elementwise arithmetic
                                and torch.sum per block
  torch_max_rel_diff            the largest relative difference of the fourteen sums (reported, not asserted: tests/test_calib_gpu.py pins
                                the kernel)
    python tools/calib_bench.py [--sizes 16384,65536] [--ks 192,256] [--iters 20] [--small 16384] [--out FILE]"""
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
    eng = ops.get_engine(0)
    lo, hi = trials.COSINE_RANGE
    g = torch.Generator(device="cuda").manual_seed(0)
    ca, cc = 8.0, -2.0

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

    def timed_ab(fa, fb, iters):
        """fa and fb alternating -> the two medians (the first round is the warm-up)."""
        ts = ([], [])
        for it in range(iters + 1):
            for k, fn in enumerate((fa, fb)):
                ms, _ = one(fn)
                if it:
                    ts[k].append(ms)
        return float(np.median(ts[0])), float(np.median(ts[1]))

    out = {"bench": "calib", "device": importlib.import_module(f"{PKG}._lib").device_info(0)["name"], "speakers": a.speakers, "point": [ca, cc],
           "score_range": [lo, hi], "cases": []}
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

            A, B = rows(la), rows(lb)
            r = torch.zeros((M,), dtype=torch.float64, device="cuda")
            calib_ms, hist_ms = timed_ab(lambda: ops_score.trial_calib(eng, A, B, r, la, sa, lb, sb, ca, cc),
                                         lambda: eng.trial_hist(A, B, r, la, sa, lb, sb, lo, hi), iters)
            dev = trials.sums_to_host(ops_score.trial_calib(eng, A, B, r, la, sa, lb, sb, ca, cc))
            trials.calibrate_scores(eng, A, B, r, la, sa, lb, sb, "cosine")                  # untimed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cal = trials.calibrate_scores(eng, A, B, r, la, sa, lb, sb, "cosine")
            fit_wall_ms = (time.perf_counter() - t0) * 1e3
            print(f"calib_bench: N=M={N} K={K}: calib {calib_ms:.2f} ms, hist {hist_ms:.2f} ms, fit {cal.n_passes} passes in {fit_wall_ms:.1f} ms "
                  f"(a {cal.a:.3f}, b {cal.b:.3f}, cllr {cal.cllr_raw:.4f} -> {cal.cllr:.4f})", file=sys.stderr, flush=True)

            blk = 2048 if N <= 16384 else 1024
            la64, lb64, sa64, sb64 = la.long(), lb.long(), sa.long(), sb.long()

            def torch_pass():
                sums = torch.zeros((2, 7), dtype=torch.float64, device="cuda")
                for i0 in range(0, N, blk):
                    S = A[i0:i0 + blk] @ B.T + r[None, :]
                    li, si = la64[i0:i0 + blk, None], sa64[i0:i0 + blk, None]
                    excl = (li < 0) | (lb64[None, :] < 0) | ((si >= 0) & (si == sb64[None, :]))
                    tgt = li == lb64[None, :]
                    z = ca * S + cc
                    m = torch.where(tgt, z, -z)
                    e = torch.exp(-m.abs())
                    d = 1.0 + e
                    p, q = e / d, 1.0 / d
                    w = torch.where(m >= 0, p, q)
                    v = p * q
                    vs = v * S
                    terms = torch.stack([(-m).clamp_min(0.0) + torch.log1p(e), w, w * S, v, vs, vs * S, S])
                    live = ~excl & torch.isfinite(S)
                    for k, mask in enumerate((live & ~tgt, live & tgt)):
                        sums[k] += (terms * mask[None]).sum(dim=(1, 2))
                return sums

            ts = torch_pass()
            torch_ms = timed(torch_pass, max(3, iters // 4))
            rel = np.abs(ts.cpu().numpy() - dev.sums) / np.maximum(np.abs(dev.sums), 1e-300)
            out["cases"].append({
                "N": N, "M": M, "K": K, "iters": iters, "trials": N * M, "n_target": int(dev.n[1]), "n_nontarget": int(dev.n[0]),
                "n_excluded": int(dev.excluded), "calib_ms": round(calib_ms, 3), "hist_ms": round(hist_ms, 3), "calib_over_hist": round(calib_ms / hist_ms, 3),
                "calib_ns_per_trial": round(calib_ms * 1e6 / (N * M), 5), "fit_passes": cal.n_passes, "fit_wall_ms": round(fit_wall_ms, 2),
                "fit_converged": bool(cal.converged), "a": float(cal.a), "b": float(cal.b), "cllr_raw": round(cal.cllr_raw, 6), "cllr": round(cal.cllr, 6),
                "min_cllr_coarse": round(cal.min_cllr_coarse, 6), "act_dcf": round(cal.act_dcf, 6), "min_dcf": round(cal.min_dcf, 6),
                "torch_ms": round(torch_ms, 3), "speedup_vs_torch": round(torch_ms / calib_ms, 2), "torch_max_rel_diff": float(rel.max())})
            del A, B
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
