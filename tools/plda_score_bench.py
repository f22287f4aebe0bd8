#!/usr/bin/env python3
"""PLDA log-likelihood-ratio scoring (sdk_plda_enroll, sdk_plda_score_topk; csrc/plda_score.hip) on one MI355X -> one JSON line.

N = 1000 windows, D = 128, S in {100, 10 000, 100 000} speakers of 1 - 5 enrolment rows each (planted: centres ~ N(0, Phi), unit noise).  Every
figure is device-event time around the one call (all launches enqueued, no host synchronisation inside), --warmup calls first, then --repeats
calls: the median and the minimum are reported.

  enroll_ms                          sdk_plda_enroll: the speaker table from the transformed profile rows
  score_ms                           sdk_plda_score_topk, k = 1, without the full matrix
  score_tflops, score_fraction_of_fp64_matrix_peak   4 N S D flop / score_ms, over FP64_MATRIX_PEAK (the datasheet's 78.6 TFLOP/s of the MI355X)
  torch_ms                           the yardstick on the same inputs: Z = [X, X^2] materialised once outside the timing, then
                                     (Z @ G.T + r).topk(1) in float64
  idx_equal_to_torch                 whether the two top-1 columns agree (planted inputs: the winners are far apart)
  identify                           one identify step of N windows against the S speakers' P profile rows on the engine's ECAPA-TDNN:
                                     embed_ms (fbank -> forward -> l2norm of N two-second windows), cosine_ms (affinity_topk over the P rows),
                                     plda_ms (plda_transform of the windows + sdk_plda_score_topk over the S speakers; the speaker table is
                                     cached per candidate set and not in it), and plda_share = (plda_ms - cosine_ms) / (embed_ms + cosine_ms):
                                     what the PLDA decision adds to the step

Prints one JSON line; the record is profiles/r29_plda_score_bench.json."""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
FP64_MATRIX_PEAK = 78.6e12


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--speakers", type=int, nargs="+", default=[100, 10000, 100000])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-identify", action="store_true", help="skip the identify-step part (no forward pass)")
    args = ap.parse_args()
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    lib = importlib.import_module(f"{PKG}._lib")
    P = importlib.import_module(f"{PKG}.plda")
    eng = ops.get_engine(0)
    N, D = args.windows, args.dim

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

    model = P.synthetic_plda(ops.EMBED_DIM, 128, lda_dim=D)
    Phi = model.device_arrays("cuda")["Phi"]
    out = {"tool": "plda_score_bench", "device": lib.device_info(0)["name"], "N": N, "D": D, "warmup": args.warmup, "repeats": args.repeats,
           "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "cases": []}
    embed_ms = None
    E = None
    if not args.no_identify:
        g = torch.Generator(device="cuda").manual_seed(1)
        pcm = (torch.randn((N, 32000), generator=g, device="cuda") * 3000).to(torch.int16)
        embed_ms = timed(lambda: eng.embed_pcm(pcm))
        E, Eb, re = eng.embed_pcm(pcm)
        rows = torch.arange(N, dtype=torch.int32, device="cuda")
    for S in args.speakers:
        g = torch.Generator(device="cuda").manual_seed(S)
        counts = torch.randint(1, 6, (S,), generator=g, device="cuda")
        group = torch.repeat_interleave(torch.arange(S, device="cuda"), counts)
        group = group[torch.randperm(group.numel(), generator=g, device="cuda")].to(torch.int32).contiguous()
        centres = torch.randn((S, D), generator=g, device="cuda", dtype=torch.float64) * Phi.sqrt()
        Xp = (centres[group.long()] + torch.randn((group.numel(), D), generator=g, device="cuda", dtype=torch.float64)).contiguous()
        X = (centres[torch.arange(N, device="cuda") % S] + torch.randn((N, D), generator=g, device="cuda", dtype=torch.float64)).contiguous()
        n_eff = counts.double()
        ms = {"enroll": timed(lambda: eng.plda_enroll(Xp, group, n_eff, Phi))}
        G, r, status = eng.plda_enroll(Xp, group, n_eff, Phi)
        ms["score"] = timed(lambda: eng.plda_score_topk(X, G, r, k=1))
        idx, sc = eng.plda_score_topk(X, G, r, k=1)
        Z = torch.cat([X, X * X], dim=1)
        ms["torch"] = timed(lambda: (Z @ G.T + r).topk(1, dim=1))
        tv, ti = (Z @ G.T + r).topk(1, dim=1)
        flop = 4.0 * N * S * D
        case = {"S": S, "P": int(group.numel()), "status": int(status.item()),
                **{f"{k}_ms": round(v[0], 4) for k, v in ms.items()}, **{f"{k}_ms_min": round(v[1], 4) for k, v in ms.items()},
                "score_tflops": round(flop / (ms["score"][0] * 1e-3) / 1e12, 3),
                "score_fraction_of_fp64_matrix_peak": round(flop / (ms["score"][0] * 1e-3) / FP64_MATRIX_PEAK, 4),
                "torch_tflops": round(flop / (ms["torch"][0] * 1e-3) / 1e12, 3),
                "idx_equal_to_torch": bool(torch.equal(idx[:, 0].long(), ti[:, 0])),
                "max_abs_diff_to_torch": float((sc[:, 0] - tv[:, 0]).abs().max())}
        if E is not None:
            g2 = torch.Generator(device="cuda").manual_seed(S + 1)
            Pn, Pb, rp = eng.l2norm(torch.randn((int(group.numel()), ops.EMBED_DIM), generator=g2, device="cuda"))
            rpm = rp.max().reshape(1)
            cos = timed(lambda: eng.affinity_topk(E, Eb, re, Pn, Pb, rpm, k=1))
            pl = timed(lambda: eng.plda_score_topk(eng.plda_transform(E, rows, model, check_rows=False), G, r, k=1))
            case["identify"] = {"embed_ms": round(embed_ms[0], 4), "cosine_ms": round(cos[0], 4), "plda_ms": round(pl[0], 4),
                                "plda_share": round((pl[0] - cos[0]) / (embed_ms[0] + cos[0]), 5)}
        out["cases"].append(case)
        del Xp, X, G, r, Z, tv, ti
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
