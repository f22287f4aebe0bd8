#!/usr/bin/env python3
"""Diarization in the ECAPA space (ecapa_diar.EcapaEmbedder) of the hour at a 1-s step of tools/diarize_bench.py (3 591 ten-second chunks,
batches of 128): one JSON line with
  stages_ms       the device stages of the whole hour, warm, event-timed: segmentation, decode + masks, fbank, the masked ECAPA forward, L2 norm
  forward         on one full batch (B = 128, T = 1001): sdk_ecapa_forward_masked at S = 3 (the hour's masks) and S = 1, and the profiler's
                  per-kernel-family split at S = 3.  The masked TAIL beside the TRUNK, as estimates (the tail's GEMMs share a family with the
                  trunk's): per slot = (S = 3 minus S = 1) / 2 (hidden + logits GEMM + pooling sweep); tail = 3 x per slot + the statistics
                  sweep + the two row FCs; trunk = S = 3 minus tail (BOTH are estimates: *_est).  Forward times: min and median of 7 windows of >= 20 ms
  three_forwards  the masked forward beside three sdk_ecapa_forward calls per chunk on the same features: what the parent commit can do
  sweeps          the two new sweeps alone (min and median of 7 event-timed windows of >= 20 ms of back-to-back launches) and their fraction of the HBM rate from the byte model: the statistics
                  sweep reads M Cm 2 bytes once for all slots, the pooling sweep M Cm (4 + 2) bytes per slot (all-ones weights: no frame is
                  skipped), against 6.3 TB/s (the figure the other tools use)
No figure is gated.  Record the line in profiles/r25_diarize_ecapa_bench.json.  Synthetic weights: the class table is the segmentation model's
own (noise-like) output."""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
HBM_BPS = 6.3e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=2)
    a = ap.parse_args()
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    seg = importlib.import_module(f"{PKG}.segmentation")
    dz = importlib.import_module(f"{PKG}.diarize")
    ed = importlib.import_module(f"{PKG}.ecapa_diar")
    lib = importlib.import_module(f"{PKG}._lib")
    eng = ops.get_engine(0)
    model, net = seg.Segmentation(eng, seg.synthetic_weights(0)), ed.EcapaEmbedder(eng)
    n = int(a.seconds * 16000)
    rng = np.random.default_rng(0)
    x = np.clip(np.round(rng.normal(0, 0.1, n) * (1 + np.sin(2 * np.pi * 0.3 * np.arange(n) / 16000)) * 32768), -32768, 32767).astype(np.int16)
    st = seg.chunk_starts(n, a.step)
    Cn, F, T = len(st), seg.num_frames(seg.CHUNK), ops.num_frames(seg.CHUNK)
    rec = torch.from_numpy(x).cuda()
    sd = torch.from_numpy(st.astype(np.int32)).cuda()
    stages = ["segmentation", "decode_masks", "fbank", "ecapa_forward_masked", "l2norm"]

    def device_pass(timed: bool):
        ev = {k: 0.0 for k in stages}
        for b0 in range(0, Cn, a.batch):
            s = sd[b0:b0 + a.batch]
            B = int(s.numel())
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            marks[0].record()
            lp = model.forward(rec, s)
            marks[1].record()
            c = dz.powerset_decode(eng, lp)
            w, info = dz.diarize_masks(eng, c, T)
            valid = info[:, :, 3].contiguous()
            marks[2].record()
            feats = eng.fbank_windows(rec.data_ptr(), n, s.data_ptr(), B, seg.CHUNK)
            marks[3].record()
            emb = net.forward_masked(feats, B, T, w, valid)
            marks[4].record()
            eng.l2norm(emb)
            marks[5].record()
            if timed:
                torch.cuda.synchronize()
                for i, k in enumerate(stages):
                    ev[k] += marks[i].elapsed_time(marks[i + 1])
        torch.cuda.synchronize()
        return ev

    device_pass(False)                                                    # warm-up: scratch buffers, code objects
    best = None
    for _ in range(a.iters):
        t0 = time.perf_counter()
        ev = device_pass(True)
        ev["device_wall"] = (time.perf_counter() - t0) * 1e3
        if best is None or ev["device_wall"] < best["device_wall"]:
            best = ev

    # one full batch: the masked forward at S = 1 and 3, three plain forwards, and the profiler's split
    B = min(a.batch, Cn)
    feats = eng.fbank_windows(rec.data_ptr(), n, sd[:B].data_ptr(), B, seg.CHUNK)
    lp = model.forward(rec, sd[:B])
    w, info = dz.diarize_masks(eng, dz.powerset_decode(eng, lp), T)
    valid = info[:, :, 3].contiguous()
    ones1, v1 = torch.ones((B, 1, T), device="cuda"), torch.ones((B, 1), dtype=torch.int32, device="cuda")

    def timed(fn, windows=7, min_ms=20.0):
        """-> (min, median) ms per call over `windows` event-timed windows, each a loop of calls long enough to last >= min_ms (short kernels
        are not timed one launch at a time), after a warm-up window"""
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        inner = max(1, int(np.ceil(min_ms / max(e0.elapsed_time(e1), 1e-3))))
        per = []
        for _ in range(windows + 1):
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) / inner)
        per = per[1:]
        return float(np.min(per)), float(np.median(per))

    (ms3, md3), (ms1, md1) = timed(lambda: eng.ecapa_forward_masked(feats, B, T, w, valid)), timed(lambda: eng.ecapa_forward_masked(feats, B, T, ones1, v1))
    (ms_plain, md_plain) = timed(lambda: eng.ecapa_forward(feats, B, T))
    (ms_three, md_three) = timed(lambda: [eng.ecapa_forward(feats, B, T) for _ in range(3)])
    eng.profile_begin()
    eng.ecapa_forward_masked(feats, B, T, w, valid)
    torch.cuda.synchronize()
    prof = eng.profile_end()

    # the two sweeps alone, all-ones weights (every frame read)
    M, Cm = B * T, eng.cfg.mfa_channels
    h = (torch.randn((M, Cm), device="cuda") * 2).to(torch.bfloat16 if eng.precision == 0 else torch.float16)
    lg = torch.randn((M, Cm), device="cuda")
    ones3, v3 = torch.ones((B, 3, T), device="cuda"), torch.ones((B, 3), dtype=torch.int32, device="cuda")
    ctx = torch.empty((B * 3, 2 * Cm), device="cuda")
    s_ = lambda: torch.cuda.current_stream().cuda_stream

    def stats():
        lib.check(eng.lib.sdk_asp_stats_masked_fmt(eng.ctx, h.data_ptr(), Cm, B, T, Cm, 3, ones3.data_ptr(), v3.data_ptr(), ctx.data_ptr(), eng.precision, s_()), "stats")

    def pool():
        lib.check(eng.lib.sdk_asp_pool_masked_fmt(eng.ctx, lg.data_ptr(), Cm, h.data_ptr(), Cm, B, T, Cm, 3, 1, ones3.data_ptr(), v3.data_ptr(), ctx.data_ptr(),
                                                  eng.precision, s_()), "pool")

    (ms_stats, md_stats), (ms_pool, md_pool) = timed(stats), timed(pool)
    slot = (ms3 - ms1) / 2
    fam = {k: round(v["ms"], 3) for k, v in prof.items() if v["ms"] > 0}
    fc = prof.get("rows_fc", {"ms": 0.0})["ms"]
    sweeps_in_fwd = prof.get("asp_stats", {"ms": 0.0})["ms"] + prof.get("asp_pool", {"ms": 0.0})["ms"]
    tail = 3 * slot + prof.get("asp_stats", {"ms": 0.0})["ms"] + fc
    out = {
        "tool": "diarize_ecapa_bench", "seconds": a.seconds, "step_s": a.step, "chunks": Cn, "batch": a.batch, "T": T, "S": 3, "precision": eng.precision,
        "timing": "per call: min | median of 7 event-timed windows of >= 20 ms each, after a warm-up window",
        "stages_ms": {k: round(v, 2) for k, v in best.items()},
        "chunks_per_s": round(Cn / (best["device_wall"] / 1e3), 1), "rtf_device": round(best["device_wall"] / 1e3 / a.seconds, 6),
        "forward": {"B": B, "masked_S3_ms": round(ms3, 3), "masked_S3_ms_median": round(md3, 3), "masked_S1_ms": round(ms1, 3), "masked_S1_ms_median": round(md1, 3),
                    "per_slot_ms_est": round(slot, 3), "tail_ms_est": round(tail, 3), "trunk_ms_est": round(ms3 - tail, 3), "families_ms": fam,
                    "sweeps_ms_in_forward": round(sweeps_in_fwd, 3)},
        "three_forwards": {"plain_forward_ms": round(ms_plain, 3), "plain_forward_ms_median": round(md_plain, 3), "three_plain_forwards_ms": round(ms_three, 3),
                           "three_plain_forwards_ms_median": round(md_three, 3), "masked_over_three": round(ms3 / ms_three, 4)},
        "sweeps": {"stats_ms": round(ms_stats, 4), "stats_ms_median": round(md_stats, 4), "stats_bytes": M * Cm * 2,
                   "stats_frac_hbm": round(M * Cm * 2 / HBM_BPS * 1e3 / ms_stats, 4), "stats_frac_hbm_median": round(M * Cm * 2 / HBM_BPS * 1e3 / md_stats, 4),
                   "pool_ms_per_slot": round(ms_pool, 4), "pool_ms_per_slot_median": round(md_pool, 4), "pool_bytes_per_slot": M * Cm * 6,
                   "pool_frac_hbm": round(M * Cm * 6 / HBM_BPS * 1e3 / ms_pool, 4), "pool_frac_hbm_median": round(M * Cm * 6 / HBM_BPS * 1e3 / md_pool, 4),
                   "hbm_bps": HBM_BPS},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
