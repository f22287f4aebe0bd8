#!/usr/bin/env python3
"""Scoring the DIHARD way on the device (score.py, csrc/score_jer.hip: evaluation maps and the Jaccard error rate) on one MI355X -> one JSON line.

  inputs    those of tools/der_bench.py: for every --configs entry RxSECONDS (default 256 x 3 min and one hour) generated reference turn lists
            (3 speakers per recording) and generated hypothesis tables (4 speakers, rows of every kind) on the packed frame grid, collar
            0.25 s.  Every recording gets a UEM of two regions: 5 % .. 45 % and 55 % .. 95 % of its length.
  calls     score.score_grouped with jer=True and the UEMs - host preparation, the one upload, seven calls and the one download - beside
            the same call without the two keywords and beside a loop of score.score_host(jer=True, uem=...) over the same recordings in
            the same process (wall clock, minimum and median of --iters windows after a warm-up), and whether every integer agrees.
  launches  the device time of sdk_score_uem, sdk_score_durations and sdk_score_jaccard alone, and of the three calls score_tables adds
            for jer=True (the two and sdk_score_map on the Jaccard table): a window of WINDOW back-to-back calls between two events, divided
            by WINDOW; minimum and median of --iters windows.
Record the line in profiles/r36_jer_bench.json.
    python tools/jer_bench.py [--configs 256x180,1x3600] [--iters 3]"""
from __future__ import annotations

import argparse
import importlib
import json
import statistics

import numpy as np

from der_bench import PKG, WINDOW, hypothesis, reference, tallies, windows


def device_ms(fn, iters: int):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    fn()
    for _ in range(iters):
        e0.record()
        for _ in range(WINDOW):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / WINDOW)
    return {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4)}


def jaccard_part(r):
    return (r.jsum, r.ref_speakers, r.jer, r.purity, r.coverage, r.ref_frames.tolist(), r.hyp_frames.tolist())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="256x180,1x3600")
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    import torch
    ops, lib, dz, sc = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "_lib", "diarize", "score"))
    eng = ops.get_engine(0)
    out = {"tool": "jer_bench", "iters": a.iters, "window": WINDOW, "scoring": []}
    for cfg in a.configs.split(","):
        R, secs = (int(v) for v in cfg.split("x"))
        n = secs * 16000
        G = dz.global_frames(n)
        refs = [reference(r, secs) for r in range(R)]
        hyps = [hypothesis(1000 + r, G) for r in range(R)]
        uems = [[(0.05 * secs, 0.45 * secs), (0.55 * secs, 0.95 * secs)] for _ in range(R)]
        tab = dz.GroupTables(eng, np.zeros(R + 1, np.int64), np.arange(R + 1, dtype=np.int64) * G, [n] * R).set_clusters(np.arange(R + 1) * 4)
        spk = torch.from_numpy(np.concatenate(hyps)).to(eng.device)
        sc.score_grouped(eng, spk, tab, refs, uems=uems, jer=True)        # warm-up: code objects
        sc.score_grouped(eng, spk, tab, refs)
        dev, t_dev = windows(lambda: sc.score_grouped(eng, spk, tab, refs, 0.25, False, uems=uems, jer=True), a.iters)
        _, t_plain = windows(lambda: sc.score_grouped(eng, spk, tab, refs, 0.25, False), a.iters)
        host, t_host = windows(lambda: [sc.score_host(h, n, t, 0.25, False, uem=u, jer=True) for h, t, u in zip(hyps, refs, uems)], a.iters)
        # the launches alone, on the tables the wrapper builds
        ref = sc.rasterise_references(eng, tab, refs, 0.25, False, uems=uems)
        merged = [sc.prepare_uem(u) for u in uems]
        uem_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(m) for m in merged])]).astype(np.int32)).to(eng.device)
        uem_d = torch.from_numpy(np.concatenate(merged).astype(np.int32)).to(eng.device)
        U = int(uem_d.shape[0])
        t = sc.score_tables(eng, spk, tab, ref, jer=True)
        co_off_d = torch.from_numpy(t.co_off).to(eng.device)
        q = torch.empty((max(int(t.co_off[-1]), 1),), dtype=torch.int32, device=eng.device)
        t_uem = device_ms(lambda: lib.check(eng.lib.sdk_score_uem(eng.ctx, uem_d.data_ptr(), uem_off.data_ptr(), tab.frame_off_d.data_ptr(), R, U, tab.G,
                                                                  ref.scored.data_ptr(), None), "sdk_score_uem"), a.iters)
        t_dur = device_ms(lambda: lib.check(eng.lib.sdk_score_durations(
            eng.ctx, ref.ref_mask.data_ptr(), ref.scored.data_ptr(), spk.data_ptr(), tab.frame_off_d.data_ptr(), ref.ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(), R,
            tab.G, ref.max_ref, 4, t.ref_frames.data_ptr(), t.hyp_frames.data_ptr(), None), "sdk_score_durations"), a.iters)
        t_jac = device_ms(lambda: lib.check(eng.lib.sdk_score_jaccard(
            eng.ctx, t.co.data_ptr(), t.ref_frames.data_ptr(), t.hyp_frames.data_ptr(), ref.ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(), co_off_d.data_ptr(), R,
            int(t.co_off[-1]), q.data_ptr(), None), "sdk_score_jaccard"), a.iters)
        t_tables = device_ms(lambda: sc.score_tables(eng, spk, tab, ref), a.iters)
        t_tables_jer = device_ms(lambda: sc.score_tables(eng, spk, tab, ref, jer=True), a.iters)
        out["scoring"].append({
            "recordings": R, "seconds_each": secs, "frames": R * G, "uem_intervals": U,
            "score_grouped_jer_uem": t_dev, "score_grouped_plain": t_plain, "score_host_loop_jer_uem": t_host,
            "jer_uem_over_plain_min": round(t_dev["min_s"] / t_plain["min_s"], 2), "speedup_over_host_min": round(t_host["min_s"] / t_dev["min_s"], 2),
            "sdk_score_uem_ms": t_uem, "sdk_score_durations_ms": t_dur, "sdk_score_jaccard_ms": t_jac,
            "score_tables_calls_ms": t_tables, "score_tables_jer_calls_ms": t_tables_jer,
            "integers_equal": bool(all(tallies(x) == tallies(y) and np.array_equal(x.co, y.co) and jaccard_part(x) == jaccard_part(y) for x, y in zip(dev, host))),
            "pooled_der": round(sc.pool(dev).der, 4), "pooled_jer": round(sc.pool(dev).jer, 4)})
        del spk, hyps, refs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
