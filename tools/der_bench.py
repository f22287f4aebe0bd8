#!/usr/bin/env python3
"""Diarization error rate on the device and the threshold sweep (score.py, csrc/score.hip, Diarizer.sweep) on one MI355X -> one JSON line.

  scoring   for every --score-configs entry RxSECONDS (default 256 x 3 min and one hour): generated reference turn lists (3 speakers per
            recording) and generated hypothesis tables (4 speakers, rows of every kind) on the packed frame grid; score.score_grouped -
            host preparation, uploads, the three kernels and the one download - beside a loop of score.score_host over the same recordings
            in the same process (wall clock, minimum and median of --iters windows after a warm-up), the device time of the three calls
            alone (a window of WINDOW back-to-back triples between two events, divided by WINDOW), and whether every tally agrees.
  sweep     --sweep-config RxSECONDS (default 256x180) of generated audio at a 1-s step, --thresholds T (default 16) thresholds spread over
            0.3 .. 1.2: Diarizer.sweep beside a loop of run_many + score_host over the same thresholds (the yardstick: the path a user
            had before), minimum and median of --iters windows each, whether the tallies agree, the sweep's per-stage split (a separate traced
            pass: every stage ended by a device synchronisation) and the waits for the device per pack.
Synthetic weights: the class table is the model's own (noise-like) output, which exercises every stage at full size; the DER figures mean
nothing, the times do not depend on them.  Record the line in profiles/r26_der_bench.json.
    python tools/der_bench.py [--score-configs 256x180,1x3600] [--sweep-config 256x180] [--thresholds 16] [--iters 3]"""
from __future__ import annotations

import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
WINDOW = 20


def recording(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n, dtype=np.float32) * np.float32(0.1) * (1 + np.sin(2 * np.pi * 0.3 * np.arange(n, dtype=np.float32) / 16000))
    return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)


def reference(seed: int, secs: float, speakers: int = 3):
    """Turns of 2 - 12 s, speaker after speaker with pauses and overlaps."""
    rng = np.random.default_rng(seed)
    t, out = 0.0, []
    while t < secs:
        d = float(rng.uniform(2.0, 12.0))
        out.append((round(t, 3), round(min(t + d, secs), 3), f"s{int(rng.integers(0, speakers))}"))
        t += d + float(rng.uniform(-1.5, 1.5))
    return out


def hypothesis(seed: int, G: int, K: int = 4) -> np.ndarray:
    rng = np.random.default_rng(seed)
    sp = np.full((G, 2), -1, np.int32)
    seg_len = 40
    first = np.repeat(rng.integers(-1, K, G // seg_len + 1), seg_len)[:G]
    second = np.repeat(rng.integers(-1, K, G // seg_len + 1), seg_len)[:G]
    sp[:, 0] = first
    ok = (first >= 0) & (second >= 0) & (second != first) & (rng.uniform(size=G) < 0.2)
    sp[ok, 1] = second[ok]
    return sp


def windows(fn, iters: int):
    import torch
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, {"min_s": round(min(ts), 5), "median_s": round(statistics.median(ts), 5)}


def tallies(r):
    return (r.scored, r.total, r.missed, r.false_alarm, r.confusion, r.correct)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--score-configs", default="256x180,1x3600")
    ap.add_argument("--sweep-config", default="256x180", help="RxSECONDS, or 'none'")
    ap.add_argument("--thresholds", type=int, default=16)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    import torch
    ops, seg, rn, dz, sc = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "segmentation", "resnet", "diarize", "score"))
    eng = ops.get_engine(0)
    out = {"tool": "der_bench", "iters": a.iters, "scoring": [], "sweep": None}
    for cfg in a.score_configs.split(","):
        R, secs = (int(v) for v in cfg.split("x"))
        n = secs * 16000
        G = dz.global_frames(n)
        refs = [reference(r, secs) for r in range(R)]
        hyps = [hypothesis(1000 + r, G) for r in range(R)]
        tab = dz.GroupTables(eng, np.zeros(R + 1, np.int64), np.arange(R + 1, dtype=np.int64) * G, [n] * R).set_clusters(np.arange(R + 1) * 4)
        spk = torch.from_numpy(np.concatenate(hyps)).to(eng.device)
        sc.score_grouped(eng, spk, tab, refs)                             # warm-up: code objects
        dev, t_dev = windows(lambda: sc.score_grouped(eng, spk, tab, refs, 0.25, False), a.iters)
        host, t_host = windows(lambda: [sc.score_host(h, n, t, 0.25, False) for h, t in zip(hyps, refs)], a.iters)
        ref = sc.rasterise_references(eng, tab, refs, 0.25, False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kern = []
        for _ in range(a.iters):
            e0.record()
            for _ in range(WINDOW):
                sc.score_tables(eng, spk, tab, ref)
            e1.record()
            torch.cuda.synchronize()
            kern.append(e0.elapsed_time(e1) / WINDOW)
        out["scoring"].append({"recordings": R, "seconds_each": secs, "frames": R * G, "score_grouped": t_dev, "score_host_loop": t_host,
                               "speedup_min": round(t_host["min_s"] / t_dev["min_s"], 2),
                               "cooccur_and_map_calls_ms": {"min": round(min(kern), 4), "median": round(statistics.median(kern), 4)},
                               "tallies_equal": bool(all(tallies(x) == tallies(y) and np.array_equal(x.co, y.co) for x, y in zip(dev, host))),
                               "pooled_der": round(sc.pool(dev).der, 4)})
        del spk, hyps, refs
    if a.sweep_config != "none":
        R, secs = (int(v) for v in a.sweep_config.split("x"))
        ths = [round(float(t), 4) for t in np.linspace(0.3, 1.2, a.thresholds)]
        diar = dz.Diarizer(eng, seg.Segmentation(eng, seg.synthetic_weights(0)), rn.ResNet34(eng, rn.synthetic_weights(0)))
        recs = [recording(r, secs * 16000) for r in range(R)]
        refs = [reference(r, secs) for r in range(R)]
        kw = dict(step_s=1.0, constrained=True)
        diar.sweep(recs[:2], refs[:2], ths[:2], **kw)                     # warm-up: code objects, scratch buffers
        diar.run_many(recs[:2], **kw)

        def loop():
            rows = []
            for t in ths:
                res = diar.run_many(recs, threshold=t, **kw)
                rows.append([sc.score_host(x.speakers, len(y), ref) for x, y, ref in zip(res, recs, refs)])
            return rows
        sw, t_sweep = windows(lambda: diar.sweep(recs, refs, ths, **kw), a.iters)
        syncs = [dict(s) for s in diar.last_sync]
        rows, t_loop = windows(loop, a.iters)
        diar.trace, diar.last_stage_s = True, []
        diar.sweep(recs, refs, ths, **kw)
        diar.trace = False
        stages = {}
        for p in diar.last_stage_s:
            for k, v in p.items():
                stages[k] = stages.get(k, 0.0) + v
        same = all(tallies(x) == tallies(y) for rs, rl in zip(sw.per_recording, rows) for x, y in zip(rs, rl))
        out["sweep"] = {"recordings": R, "seconds_each": secs, "thresholds": ths, "packs": len(syncs), "sweep": t_sweep, "run_many_score_host_loop": t_loop,
                        "speedup_min": round(t_loop["min_s"] / t_sweep["min_s"], 2), "tallies_equal_the_loop": bool(same),
                        "sweep_stage_ms_traced": {k: round(v * 1e3, 2) for k, v in stages.items()}, "waits_for_the_device_per_pack": syncs[0],
                        "pooled_der": [round(p.der, 4) for p in sw.pooled], "best": sw.thresholds[sw.best]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
